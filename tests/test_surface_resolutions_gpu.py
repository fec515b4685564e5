"""GPU tests of point and mesh extraction (vbg_extract.hip, vbg_mesh.hip) at
every block-resolution form vbg_surface.h's WithRes picks: compile-time 16
and 8, a run-time power of two (mask and shift) and any other run-time value
(% and /). Grids come from _surface_grids.sphere_blocks through
VoxelBlockGrid.load: absent neighbours and negative keys. Results are
compared byte for byte, in order, with the C oracle's ExtractPointCloud and
with the numpy mesh restatement (tests/_mesh_oracle.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _oracle as orc
import _surface_grids as sg
from test_mesh_gpu import _assert_equal, _oracle as _mesh_oracle, _write_npz
from test_slam_gpu import _nb_tables

pytestmark = pytest.mark.gpu

POINT_RES = [1, 2, 3, 4, 5, 7, 12, 32, 64]
MESH_RES = [1, 2, 3, 4, 5, 7, 12, 32]


def _geometry():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import geometry
    return geometry


def _grid(tmp_path, res, wdt, with_color, edge_values=False, seed=0,
          thresholds=(3.0, 10.0)):
    geometry = _geometry()
    keys, tsdf, w, c = sg.sphere_blocks(res, wdt, with_color, seed=seed,
                                        edge_values=edge_values,
                                        thresholds=thresholds)
    p = str(tmp_path / ("g%d.npz" % res))
    _write_npz(p, keys, tsdf, w, c, res)
    g = geometry.VoxelBlockGrid.load(p)
    assert g.block_resolution == res
    assert g.hashmap().size() == keys.shape[0]
    return g


def _points_oracle(g, thr):
    hm = g.hashmap()
    active = np.sort(hm.active_buf_indices().cpu().numpy())
    nbi, nbm = _nb_tables(hm, active)
    col = g.attribute("color").cpu().numpy() \
        if "color" in g.attr_names else None
    return orc.extract_point_cloud(
        active, nbi, nbm, hm.key_tensor().cpu().numpy(),
        g.attribute("tsdf").cpu().numpy()[..., 0],
        g.attribute("weight").cpu().numpy()[..., 0], col,
        g.block_resolution, np.float32(g.voxel_size), thr)


def _assert_points(got, want):
    assert got["positions"].shape[0] == want[3]
    assert got["positions"].cpu().numpy().tobytes() == want[0].tobytes()
    assert got["normals"].cpu().numpy().tobytes() == want[1].tobytes()
    assert ("colors" in got) == (want[2] is not None)
    if want[2] is not None:
        assert got["colors"].cpu().numpy().tobytes() == want[2].tobytes()


@pytest.mark.parametrize("res", POINT_RES)
@pytest.mark.parametrize("wdt", [np.float32, np.uint16])
def test_point_cloud_at_every_resolution_form(tmp_path, res, wdt):
    g = _grid(tmp_path, res, wdt, with_color=wdt == np.uint16)
    for thr in (3.0, 10.5):
        want = _points_oracle(g, thr)
        assert want[3] > 100
        _assert_points(g.extract_point_cloud(thr), want)


@pytest.mark.parametrize("res", MESH_RES)
@pytest.mark.parametrize("wdt", [np.float32, np.uint16])
def test_triangle_mesh_at_every_resolution_form(tmp_path, res, wdt):
    """At R = 1 the normal at an edge's far end reads offset 2R, which the
    GPU folds into the +1 neighbour as the reference does."""
    g = _grid(tmp_path, res, wdt, with_color=wdt == np.uint16)
    for thr in (3.0, 10.5):
        want = _mesh_oracle(g, thr)
        assert want["indices"].shape[0] > 50
        _assert_equal(g.extract_triangle_mesh(thr), want)


@pytest.mark.parametrize("res", [4, 5, 16])
@pytest.mark.parametrize("wdt", [np.float32, np.uint16])
def test_surfaces_with_signed_zeros_and_weights_at_threshold(tmp_path, res,
                                                             wdt):
    """Crossings through tsdf +0.0 and -0.0 (a point needs a product < 0, a
    mesh corner is inside when tsdf < 0) and through integer weights equal to
    the threshold (not above it: no point, no cube)."""
    thresholds = (3.0, 10.0)
    g = _grid(tmp_path, res, wdt, with_color=True, edge_values=True,
              thresholds=thresholds)
    active = g.hashmap().active_buf_indices().cpu().numpy()
    assert sg.has_edge_values(g.attribute("tsdf").cpu().numpy()[active],
                              g.attribute("weight").cpu().numpy()[active],
                              thresholds)
    for thr in thresholds:
        want = _points_oracle(g, thr)
        assert want[3] > 50
        _assert_points(g.extract_point_cloud(thr), want)
        want = _mesh_oracle(g, thr)
        assert want["indices"].shape[0] > 50
        _assert_equal(g.extract_triangle_mesh(thr), want)


def test_capacity_at_a_run_time_resolution(tmp_path):
    g = _grid(tmp_path, 12, np.uint16, True)
    full = g.extract_point_cloud(3.0)
    n = full["positions"].shape[0]
    _assert_points(full, _points_oracle(g, 3.0))
    part = g.extract_point_cloud(3.0, n // 3)
    assert part["positions"].shape[0] == n // 3
    for k in ("positions", "normals", "colors"):
        assert torch.equal(part[k], full[k][:n // 3]), k

    mesh = g.extract_triangle_mesh(3.0)
    nv = mesh["positions"].shape[0]
    want = {k: v.cpu().numpy() for k, v in mesh.items()}
    _assert_equal(mesh, _mesh_oracle(g, 3.0))
    with pytest.raises(RuntimeError,
                       match="estimated_vertex_number too small"):
        g.extract_triangle_mesh(3.0, nv - 1)
    _assert_equal(g.extract_triangle_mesh(3.0, nv), want)


def _refused(call, n_counts):
    from open3d_amd import _lib
    counts = [C.c_int64(77) for _ in range(n_counts)]
    st = call(*[C.byref(c) for c in counts])
    msg = _lib.lib().o3dmi_last_error().decode()
    return st, msg, [c.value for c in counts]


@pytest.mark.parametrize("res", [33, 65])
def test_resolution_limits(tmp_path, res):
    """Point extraction takes R up to 64, mesh extraction up to 32 (R = 64
    and 32 pass above); past that the seam refuses and the counts read 0."""
    from open3d_amd import _lib
    from open3d_amd.core import stream
    L = _lib.lib()
    geometry = _geometry()
    keys, tsdf, w, _ = sg.sphere_blocks(res, np.float32, False)
    near = np.argsort(-(np.abs(tsdf) < 1.0 / res).sum(1))[:2]
    keys, tsdf, w = keys[near], tsdf[near], w[near]
    p = str(tmp_path / "big.npz")
    _write_npz(p, keys, tsdf, w, None, res)
    g = geometry.VoxelBlockGrid.load(p)
    st, msg, (nv, nt) = _refused(
        lambda a, b: L.o3dmi_vbg_extract_triangle_mesh(
            g._g, C.c_float(3.0), C.c_int64(-1), None, None, None, None, a, b,
            stream()), 2)
    assert st == 1, st  # O3DMI_ERR_INVALID_ARG
    assert "block resolution must be in [1, 32]" in msg, msg
    assert (nv, nt) == (0, 0)
    if res == 65:
        st, msg, (total,) = _refused(
            lambda a: L.o3dmi_vbg_extract_point_cloud(
                g._g, C.c_float(3.0), C.c_int64(-1), None, None, None, a,
                stream()), 1)
        assert st == 1 and "bad block resolution" in msg, (st, msg)
        assert total == 0
    else:
        _assert_points(g.extract_point_cloud(3.0), _points_oracle(g, 3.0))
