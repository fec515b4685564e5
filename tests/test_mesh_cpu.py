"""CPU checks of VoxelBlockGrid::ExtractTriangleMesh's ground: the generated
marching-cubes table (tools/gen_mc_tables.py -> open3d_amd/csrc/mc_tables.h)
against what the reference's table implies, and the CPU restatement
(tests/_mesh_oracle.py) on hand-computed volumes."""
import os
import sys

import numpy as np
import pytest

import _mesh_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_MACROS = ("/root/reference/cpp/open3d/t/geometry/kernel/"
              "GeometryMacros.h")

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, GOLDEN)
import gen_mc_tables as gen  # noqa: E402
import make_mc_golden as mk  # noqa: E402


def _reference_topology():
    if os.path.exists(REF_MACROS):
        d = mk.derive(REF_MACROS)
        z = np.load(os.path.join(GOLDEN, "mc_reference_topology.npz"))
        for k in ("edge_mask", "tri_count", "boundary"):
            assert np.array_equal(z[k], d[k]), "stale fixture: " + k
        return d
    z = np.load(os.path.join(GOLDEN, "mc_reference_topology.npz"))
    return {k: z[k] for k in z.files}


def test_table_matches_the_reference_topology():
    ref = _reference_topology()
    edge, tri, cnt = gen.tables()
    assert np.array_equal(edge, ref["edge_mask"])
    assert np.array_equal(cnt, ref["tri_count"])
    b = ref["boundary"]
    for case in range(256):
        t = tri[case, :3 * cnt[case]].reshape(-1, 3)
        mine = mk.boundary_edges(t)
        want = b[b[:, 0] == case][:, 1:]
        assert np.array_equal(mine, want), case


def test_table_triangles_are_well_formed():
    edge, tri, cnt = gen.tables()
    for case in range(256):
        t = tri[case, :3 * cnt[case]].reshape(-1, 3)
        assert (tri[case, 3 * cnt[case]:] == -1).all()
        for a, b_, c in t:
            assert len({a, b_, c}) == 3
            for e in (a, b_, c):
                assert (edge[case] >> e) & 1, (case, e)
        # every crossing edge is used, nothing else
        used = set(t.reshape(-1).tolist())
        assert used == {j for j in range(12) if (edge[case] >> j) & 1}


def test_header_is_not_stale():
    with open(gen.HEADER) as f:
        assert f.read() == gen.render()


# ---------------------------------------------------------------- volumes
def _grid(block_keys, res, fn, weight=10.0):
    """keys {n,3}, tsdf / weight {n, R^3} with tsdf = fn(x, y, z) of the
    global voxel coordinates; buffer index = row."""
    keys = np.asarray(block_keys, np.int32)
    v = np.arange(res ** 3)
    lx, ly, lz = v % res, (v // res) % res, v // (res * res)
    X = keys[:, :1] * res + lx
    Y = keys[:, 1:2] * res + ly
    Z = keys[:, 2:] * res + lz
    tsdf = fn(X, Y, Z).astype(np.float32)
    w = np.full(tsdf.shape, weight, np.float32)
    return keys, tsdf, w


def _blocks(nx, ny, nz, origin=(0, 0, 0)):
    return [(origin[0] + i, origin[1] + j, origin[2] + k)
            for k in range(nz) for j in range(ny) for i in range(nx)]


def test_plane_vertices_and_normals():
    res, c = 8, 5.25
    keys, tsdf, w = _grid(_blocks(2, 2, 2), res,
                          lambda x, y, z: (z - c) / 4.0)
    out = mo.extract_triangle_mesh(keys, np.arange(len(keys)), tsdf, w, None,
                                   res, 1.0, 3.0)
    P, N, T = out["positions"], out["normals"], out["indices"]
    assert P.shape[0] > 0 and T.shape[0] > 0
    assert (P[:, 2] == np.float32(c)).all()
    # (0, 0, 1) up to the reference's n / (|n| + 1e-5)
    assert (N[:, :2] == 0).all()
    assert np.allclose(N[:, 2], 1, atol=1e-4)
    # every face normal points to +z (towards tsdf > 0)
    fn = np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
    assert (fn[:, 2] > 0).all()


def _sphere(res=8, r=6.3, centre=(8.1, 7.9, 8.2)):
    cx, cy, cz = centre
    return _grid(_blocks(2, 2, 2), res, lambda x, y, z: np.sqrt(
        (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r)


def _check_closed_manifold(T, nv):
    assert T.shape[0] > 0
    assert (T >= 0).all() and (T < nv).all()
    assert (T[:, 0] != T[:, 1]).all() and (T[:, 1] != T[:, 2]).all() and \
        (T[:, 0] != T[:, 2]).all()
    d = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    key = d[:, 0].astype(np.int64) * nv + d[:, 1]
    assert np.unique(key).shape[0] == key.shape[0], "directed edge twice"
    rev = d[:, 1].astype(np.int64) * nv + d[:, 0]
    assert np.isin(rev, key).all(), "edge without its opposite"
    E = key.shape[0] // 2
    used = np.unique(T).shape[0]
    assert used == nv
    assert nv - E + T.shape[0] == 2


def test_sphere_is_a_closed_oriented_manifold():
    keys, tsdf, w = _sphere()
    out = mo.extract_triangle_mesh(keys, np.arange(len(keys)), tsdf, w, None,
                                   8, 0.5, 3.0)
    P, N, T = out["positions"], out["normals"], out["indices"]
    _check_closed_manifold(T, P.shape[0])
    # face normals agree in sign with the interpolated vertex normals
    fn = np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
    vn = N[T].sum(axis=1)
    assert ((fn * vn).sum(axis=1) > 0).all()
    # and point outwards (tsdf grows outwards)
    centre = np.float32(0.5) * np.array([8.1, 7.9, 8.2], np.float32)
    assert ((fn * (P[T].mean(axis=1) - centre)).sum(axis=1) > 0).all()


def test_weight_at_threshold_produces_no_cube():
    res = 8
    keys, tsdf, w = _grid(_blocks(1, 1, 1), res,
                          lambda x, y, z: (z - 3.5) + 0 * x)
    full = mo.extract_triangle_mesh(keys, [0], tsdf, w, None, res, 1.0, 3.0)
    # voxel (2, 2, 3): one corner of the cubes at (1..2, 1..2, 2..3)
    w2 = w.copy()
    w2[0, (3 * res + 2) * res + 2] = 3.0  # == threshold: not > threshold
    cut = mo.extract_triangle_mesh(keys, [0], tsdf, w2, None, res, 1.0, 3.0)
    assert cut["indices"].shape[0] == full["indices"].shape[0] - 2 * 4
    w2[0, (3 * res + 2) * res + 2] = np.nextafter(np.float32(3), np.float32(4))
    back = mo.extract_triangle_mesh(keys, [0], tsdf, w2, None, res, 1.0, 3.0)
    assert back["indices"].shape[0] == full["indices"].shape[0]
