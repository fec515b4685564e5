"""GPU tests of VoxelBlockGrid::ExtractTriangleMesh / slam::Model::
ExtractTriangleMesh (open3d_amd/csrc/vbg_mesh.hip) against the CPU
restatement of the reference's passes 0-3 (tests/_mesh_oracle.py) run with
the project's generated table: positions, normals, colours and triangle
indices array-equal, in order."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mesh_oracle as mo
import _scene as sc
from test_mesh_cpu import _check_closed_manifold
from test_vbg_gpu import _mk_grid

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib, geometry, slam
    return _lib, geometry, slam


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _write_npz(path, keys, tsdf, weight, color, res, voxel=0.01):
    n = keys.shape[0]
    d = {"voxel_size": np.array([voxel], np.float32),
         "block_resolution": np.array([res], np.int64),
         "CUDA:0": np.zeros((), np.uint8),
         "attr_name_tsdf": np.array([0], np.int32),
         "attr_name_weight": np.array([1], np.int32),
         "key": keys.astype(np.int32),
         "value_000": tsdf.reshape(n, res, res, res, 1),
         "value_001": weight.reshape(n, res, res, res, 1)}
    if color is not None:
        d["attr_name_color"] = np.array([2], np.int32)
        d["value_002"] = color.reshape(n, res, res, res, 3)
    np.savez(path, **d)


def _sphere_grid(tmp_path, res, wdt, with_color, seed=0, name="g.npz"):
    """Blocks of a 3x3x3 cube of blocks minus a few, a sphere crossing block
    faces and corners, weights scattered around the thresholds."""
    _, geometry, _ = _gpu()
    rng = np.random.default_rng(seed)
    keys = np.array([(i, j, k) for k in range(-1, 2) for j in range(-1, 2)
                     for i in range(-1, 2)], np.int32)
    keys = keys[rng.permutation(len(keys))[:24]]
    v = np.arange(res ** 3)
    X = keys[:, :1] * res + v % res
    Y = keys[:, 1:2] * res + (v // res) % res
    Z = keys[:, 2:] * res + v // (res * res)
    r = 1.1 * res
    tsdf = (np.sqrt((X - 0.3) ** 2 + (Y + 0.2) ** 2 + (Z - 0.1) ** 2) - r) / res
    tsdf = (tsdf + 0.02 * rng.standard_normal(tsdf.shape)).astype(np.float32)
    w = rng.integers(0, 12, tsdf.shape)
    w[rng.random(tsdf.shape) < 0.9] = 20
    weight = w.astype(wdt)
    color = rng.integers(0, 256, tsdf.shape + (3,)).astype(wdt) \
        if with_color else None
    p = str(tmp_path / name)
    _write_npz(p, keys, tsdf, weight, color, res)
    return geometry.VoxelBlockGrid.load(p)


def _oracle(g, thr):
    hm = g.hashmap()
    R = g.block_resolution
    cap = hm.capacity()
    active = np.sort(hm.active_buf_indices().cpu().numpy())
    col = g.attribute("color").cpu().numpy().reshape(cap, R ** 3, 3) \
        if "color" in g.attr_names else None
    return mo.extract_triangle_mesh(
        hm.key_tensor().cpu().numpy(), active,
        g.attribute("tsdf").cpu().numpy().reshape(cap, -1),
        g.attribute("weight").cpu().numpy().reshape(cap, -1), col, R,
        np.float32(g.voxel_size), thr)


def _assert_equal(got, want):
    for k in ("positions", "normals", "colors", "indices"):
        assert (k in got) == (k in want), k
        if k not in want:
            continue
        a = got[k].cpu().numpy()
        assert a.shape == want[k].shape, (k, a.shape, want[k].shape)
        assert a.dtype == want[k].dtype, k
        assert a.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("res", [16, 8])
@pytest.mark.parametrize("wdt", [np.float32, np.uint16])
@pytest.mark.parametrize("with_color", [True, False])
def test_matches_the_restatement(tmp_path, res, wdt, with_color):
    g = _sphere_grid(tmp_path, res, wdt, with_color)
    for thr in (3.0, 10.5):
        want = _oracle(g, thr)
        got = g.extract_triangle_mesh(thr)
        assert want["indices"].shape[0] > 100
        _assert_equal(got, want)


def test_integrated_grid_matches_the_restatement():
    _, geometry, _ = _gpu()
    g = _mk_grid(geometry, False, block_count=8192)
    for k in range(100, 106):
        d, c, K, Ts = sc.frames(k * 3, 1, 320, 240)
        g.integrate_frame(_dev(d[0]), _dev(c[0]), K, K, Ts[0])
    assert g.hashmap().size() > 300
    want = _oracle(g, 1.0)
    got = g.extract_triangle_mesh(1.0)
    assert want["indices"].shape[0] > 1000
    _assert_equal(got, want)


def test_sphere_across_blocks_is_watertight(tmp_path):
    _, geometry, _ = _gpu()
    res = 8
    keys = np.array([(i, j, k) for k in range(-2, 2) for j in range(-2, 2)
                     for i in range(-2, 2)], np.int32)
    v = np.arange(res ** 3)
    X = keys[:, :1] * res + v % res
    Y = keys[:, 1:2] * res + (v // res) % res
    Z = keys[:, 2:] * res + v // (res * res)
    # centred on a block corner: the surface crosses faces, edges, corners
    tsdf = (np.sqrt((X + 0.1) ** 2 + (Y - 0.2) ** 2 + (Z + 0.3) ** 2) -
            11.7).astype(np.float32)
    w = np.full(tsdf.shape, 50, np.float32)
    p = str(tmp_path / "s.npz")
    _write_npz(p, keys, tsdf, w, None, res)
    g = geometry.VoxelBlockGrid.load(p)
    got = g.extract_triangle_mesh(3.0)
    P = got["positions"].cpu().numpy()
    T = got["indices"].cpu().numpy()
    _check_closed_manifold(T, P.shape[0])
    _assert_equal(got, _oracle(g, 3.0))


def test_two_calls_give_the_same_bits(tmp_path):
    g = _sphere_grid(tmp_path, 16, np.uint16, True)
    a = g.extract_triangle_mesh(3.0)
    b = g.extract_triangle_mesh(3.0)
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes()


def test_empty_grid():
    _, geometry, _ = _gpu()
    g = _mk_grid(geometry, False, block_count=256)
    out = g.extract_triangle_mesh(3.0)
    assert out["positions"].shape == (0, 3)
    assert out["normals"].shape == (0, 3)
    assert out["colors"].shape == (0, 3)
    assert out["indices"].shape == (0, 3) and \
        out["indices"].dtype == torch.int32
    assert g.extract_triangle_mesh(3.0, 10)["indices"].shape == (0, 3)


def test_estimated_vertex_number(tmp_path):
    _lib, _, _ = _gpu()
    g = _sphere_grid(tmp_path, 8, np.float32, True)
    full = g.extract_triangle_mesh(3.0)
    nv, nt = full["positions"].shape[0], full["indices"].shape[0]
    exact = g.extract_triangle_mesh(3.0, nv)
    _assert_equal(exact, {k: v.cpu().numpy() for k, v in full.items()})
    big = g.extract_triangle_mesh(3.0, nv + 1000)
    _assert_equal(big, {k: v.cpu().numpy() for k, v in full.items()})
    with pytest.raises(RuntimeError):
        g.extract_triangle_mesh(3.0, nv - 1)
    # too small: O3DMI_ERR_CAPACITY and nothing written, not even in range
    cap, guard = nv - 1, 4096
    bufs = [torch.full(((cap + guard) * 3,), -7.0, device="cuda")
            for _ in range(3)]
    tri = torch.full((3 * (cap + guard) * 3,), -7, dtype=torch.int32,
                     device="cuda")
    cnt_v, cnt_t = C.c_int64(0), C.c_int64(0)
    torch.cuda.synchronize()
    st = _lib.lib().o3dmi_vbg_extract_triangle_mesh(
        g._g, C.c_float(3.0), C.c_int64(cap), _lib.ptr(bufs[0]),
        _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), _lib.ptr(tri), C.byref(cnt_v),
        C.byref(cnt_t), None)
    torch.cuda.synchronize()
    assert st == 3  # O3DMI_ERR_CAPACITY
    assert (cnt_v.value, cnt_t.value) == (nv, nt)
    for b in bufs:
        assert (b == -7.0).all()
    assert (tri == -7).all()
    assert nt <= 3 * nv


def test_model_extract_trianglemesh_equals_the_grid():
    _, _, slam = _gpu()
    d, c, K, Ts = sc.frames(0, 3, 320, 240)
    model = slam.Model(sc.VOXEL, sc.RES, 4096)
    f = slam.Frame(240, 320, K)
    for i in range(3):
        model.update_frame_pose(i, np.linalg.inv(np.array(Ts[i])))
        f.set_data_from_image("depth", _dev(d[i]))
        f.set_data_from_image("color", _dev(c[i]))
        model.integrate(f)
    a = model.extract_trianglemesh(1.0)
    b = model.voxel_grid.extract_triangle_mesh(1.0)
    assert a["indices"].shape[0] > 1000
    assert set(a) == {"positions", "normals", "colors", "indices"}
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes()


def test_grid_past_the_int32_linear_index():
    """524 288 blocks of 16^3 = 2^31 voxels: a plane through one layer of
    blocks. The count equals the restatement's per-block sums, taken on a
    2 x 2 layout of the same blocks (interior / +x edge / +y edge / corner)."""
    _, geometry, _ = _gpu()
    res, nx, ny = 16, 1024, 512
    n = nx * ny
    need = n * res ** 3 * (4 + 4 + 4) + n * res ** 2 * 100
    free, _ = torch.cuda.mem_get_info()
    if free < need * 1.3:
        pytest.skip("device short of memory (%d GB free)" % (free >> 30))
    small = mo.extract_triangle_mesh(
        np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], np.int32),
        np.arange(4),
        *_plane_blocks(np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]),
                       res), None, res, 0.01, 3.0)
    bv, bt = small["block_vertices"], small["block_triangles"]
    want_v = n * int(bv[0])
    assert (bv == bv[0]).all()
    want_t = (nx - 1) * (ny - 1) * int(bt[0]) + (ny - 1) * int(bt[1]) + \
        (nx - 1) * int(bt[2]) + int(bt[3])
    g = _big_plane_grid(geometry, nx, ny, res)
    assert g.hashmap().size() == n
    from open3d_amd import _lib as L
    nv, nt = C.c_int64(0), C.c_int64(0)
    st = L.lib().o3dmi_vbg_extract_triangle_mesh(
        g._g, C.c_float(3.0), C.c_int64(-1), None, None, None, None,
        C.byref(nv), C.byref(nt), None)
    assert st == 0
    assert (nv.value, nt.value) == (want_v, want_t)
    out = g.extract_triangle_mesh(3.0)
    assert out["positions"].shape[0] == want_v
    T = out["indices"]
    assert T.shape[0] == want_t
    assert int(T.min()) >= 0 and int(T.max()) == want_v - 1
    z = out["positions"][:, 2]
    assert bool((z == np.float32(0.01) * np.float32(7.25)).all())
    del out, T, z, g
    torch.cuda.empty_cache()


def _plane_blocks(keys, res):
    v = np.arange(res ** 3)
    Z = keys[:, 2:] * res + v // (res * res)
    tsdf = np.broadcast_to((Z - 7.25) / 4.0, (len(keys), res ** 3))
    return (np.ascontiguousarray(tsdf, np.float32),
            np.full((len(keys), res ** 3), 10, np.float32))


def _big_plane_grid(geometry, nx, ny, res):
    """One layer of nx x ny blocks: activated with merge_blocks in chunks,
    then the rows written through the attribute views."""
    g = geometry.VoxelBlockGrid(["tsdf", "weight"],
                                [torch.float32, torch.float32], [1, 1],
                                voxel_size=0.01, block_resolution=res,
                                block_count=nx * ny + 4096)
    j, i = torch.meshgrid(torch.arange(ny, device="cuda"),
                          torch.arange(nx, device="cuda"), indexing="ij")
    keys = torch.stack([i.reshape(-1), j.reshape(-1),
                        torch.zeros_like(i.reshape(-1))], 1).int()
    chunk = 16384
    r3 = res ** 3
    for s in range(0, keys.shape[0], chunk):
        k = keys[s:s + chunk].contiguous()
        m = k.shape[0]
        g.merge_blocks(k, [torch.zeros(m * r3, device="cuda"),
                           torch.zeros(m * r3, device="cuda")])
    tsdf = g.attribute("tsdf").view(-1, r3)
    wgt = g.attribute("weight").view(-1, r3)
    z = (torch.arange(r3, device="cuda") // (res * res)).float()
    row = ((z - 7.25) / 4.0).float()
    act = g.hashmap().active_buf_indices().long()
    for s in range(0, act.shape[0], chunk):
        a = act[s:s + chunk]
        tsdf[a] = row.expand(a.shape[0], r3)
        wgt[a] = 10.0
    torch.cuda.synchronize()
    return g
