"""slac::ControlGrid on the MI355X against the numpy restatement
(tests/_control_grid_oracle.py). Buffer indices are the hash's business: every
comparison of indices goes through the key tensor."""
import functools

import numpy as np
import pytest
import torch

import _control_grid_oracle as co
import _scene

pytestmark = pytest.mark.gpu

F = np.float32
GRID = 0.375
INVALID_ARG = 1
W, H = 80, 60
SCALE, DMAX = _scene.DEPTH_SCALE, _scene.DEPTH_MAX


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F else a.dtype)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.count_nonzero(g != w)
    assert bad == 0, "%s: %d of %d words differ" % (what, bad, g.size)


@functools.lru_cache(maxsize=None)
def _cloud(n=1500, seed=11):
    """A 1.5 m box that straddles the origin; the first rows lie exactly on
    lattice planes."""
    rng = np.random.RandomState(seed)
    p = rng.uniform(-0.75, 0.75, (n, 3)).astype(F)
    p[:40, 0] = (rng.randint(-2, 2, 40) * GRID).astype(F)
    p[20:60, 1] = (rng.randint(-2, 2, 40) * GRID).astype(F)
    p[50:90, 2] = (rng.randint(-2, 2, 40) * GRID).astype(F)
    nm = rng.normal(size=(n, 3))
    nm = (nm / np.linalg.norm(nm, axis=1, keepdims=True)).astype(F)
    cl = rng.uniform(0, 1, (n, 3)).astype(F)
    return p, nm, cl


def _touched(points, grid_count=1000):
    from open3d_amd import slac
    g = slac.ControlGrid(GRID, grid_count)
    g.touch(_cuda(points))
    return g


def _nodes(g):
    """(active buffer indices, their keys, their current positions), rows
    sorted by key."""
    hm = g.get_hashmap()
    act = hm.active_buf_indices().long()
    keys = hm.key_tensor()[act].cpu().numpy()
    curr = g.get_curr_positions()[act].cpu().numpy()
    order = np.lexsort(keys.T[::-1])
    return act.cpu().numpy()[order], keys[order], curr[order]


def _grid_dict(g):
    _, keys, curr = _nodes(g)
    return {tuple(int(v) for v in k): c for k, c in zip(keys, curr)}


def _displace(g):
    init = g.get_init_positions()
    g.get_curr_positions().copy_(init + 0.02 * torch.sin(init))


def _keys_of(g, indices):
    return g.get_hashmap().key_tensor()[indices.long().reshape(-1)] \
        .cpu().numpy().reshape(tuple(indices.shape) + (3,))


# ---- touch ------------------------------------------------------------------

def test_touch_creates_the_oracles_nodes():
    p, _, _ = _cloud()
    want_keys, want_vals = co.touch(p, GRID)
    assert (want_keys < 0).any() and (want_keys > 0).any()
    g = _touched(p)
    _, keys, curr = _nodes(g)
    assert g.size() == len(want_keys)
    assert np.array_equal(keys, want_keys)
    _same(curr, want_vals, "values")
    _same(curr, keys.astype(F) * F(GRID), "key * grid_size")
    g.touch(_cuda(p))  # again: nothing new, nothing moved
    _, keys2, curr2 = _nodes(g)
    assert g.size() == len(want_keys) and np.array_equal(keys2, keys)
    _same(curr2, curr, "values after the second touch")
    _, keys3, curr3 = _nodes(_touched(p))
    assert np.array_equal(keys3, keys)
    _same(curr3, curr, "a second grid")


def test_touch_grows_a_small_grid_and_loses_no_node():
    p, _, _ = _cloud()
    want_keys, want_vals = co.touch(p, GRID)
    assert len(want_keys) > 100
    g = _touched(p, grid_count=16)
    _, keys, curr = _nodes(g)
    assert g.get_hashmap().capacity() >= len(want_keys)
    assert np.array_equal(keys, want_keys)
    _same(curr, want_vals, "values")


def test_touch_ignores_non_finite_rows():
    p, _, _ = _cloud()
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.2, -np.inf],
                    [np.nan, np.nan, np.nan], [3e38, 0, 0], [0, -1e12, 0]], F)
    mixed = np.concatenate([bad[:3], p, bad[3:]])
    want_keys, _ = co.touch(p, GRID)
    assert np.array_equal(co.touch(mixed, GRID)[0], want_keys)
    _, keys, _ = _nodes(_touched(mixed))
    assert np.array_equal(keys, want_keys)
    g = _touched(bad)
    assert g.size() == 0


# ---- compactify -------------------------------------------------------------

def test_compactify_keeps_the_contents_and_picks_the_median_anchor():
    p, _, _ = _cloud()
    g = _touched(p, grid_count=2000)
    _displace(g)
    _, keys, curr = _nodes(g)
    g.compactify()
    _, keys2, curr2 = _nodes(g)
    assert np.array_equal(keys2, keys)
    _same(curr2, curr, "values")
    assert g.get_hashmap().capacity() >= 2 * g.size()
    anchor = g.get_anchor_idx()
    key = g.get_hashmap().key_tensor()[anchor].cpu().numpy()
    assert tuple(int(v) for v in key) == co.anchor_key(keys)
    g.compactify()
    key = g.get_hashmap().key_tensor()[g.get_anchor_idx()].cpu().numpy()
    assert tuple(int(v) for v in key) == co.anchor_key(keys)


# ---- neighbour map ----------------------------------------------------------

def test_neighbor_grid_map():
    p, _, _ = _cloud(400, 12)  # a sparser cloud: some cells stay empty
    g = _touched(p[:120] * F(2))
    active, nb, masks = g.get_neighbor_grid_map()
    keys = _keys_of(g, active)
    assert len(keys) == g.size()
    want = co.neighbor_masks(keys)
    assert want.any() and not want.all()
    assert np.array_equal(masks.cpu().numpy(), want)
    nb_keys = _keys_of(g, nb)
    expect = keys[:, None, :] + co.DIRECTIONS[None]
    assert np.array_equal(nb_keys[want], expect[want])
    assert (nb.cpu().numpy()[~want] == 0).all()
    a2, nb2, m2 = g.get_neighbor_grid_map()
    assert torch.equal(a2, active) and torch.equal(nb2, nb) and \
        torch.equal(m2, masks)


# ---- parameterize -----------------------------------------------------------

def _mixed_cloud():
    """Two thirds inside the touched box, a third outside it: far away, and
    just past its border where only some corners exist."""
    p, nm, cl = _cloud()
    rng = np.random.RandomState(13)
    out = p[:750].copy()
    out[:400, 0] += F(3.0)
    out[400:, 1] = rng.uniform(0.76, 1.1, 350).astype(F)
    pts = np.concatenate([p, out])
    perm = rng.permutation(len(pts))
    return (pts[perm], np.concatenate([nm, nm[:750]])[perm],
            np.concatenate([cl, cl[:750]])[perm])


def _check_parameterize(with_normals):
    p, _, _ = _cloud()
    pts, nm, cl = _mixed_cloud()
    g = _touched(p)
    nodes = co.key_set(co.touch(p, GRID)[0])
    want = co.parameterize(pts, GRID, nodes, nm if with_normals else None)
    n_valid = int(want["valid"].sum())
    assert n_valid == len(p), "the inside points and no others"
    got = g.parameterize(_cuda(pts), _cuda(nm) if with_normals else None,
                         _cuda(cl))
    assert got.positions.shape[0] == n_valid
    _same(got.positions, pts[want["valid"]], "positions (input order)")
    _same(got.colors, cl[want["valid"]], "colors")
    assert np.array_equal(_keys_of(g, got.Grid8NbIndices), want["keys"])
    _same(got.Grid8NbVertexInterpRatios, want["vertex"], "vertex ratios")
    if with_normals:
        _same(got.normals, nm[want["valid"]], "normals")
        _same(got.Grid8NbNormalInterpRatios, want["normal"], "normal ratios")
    else:
        assert got.normals is None and got.Grid8NbNormalInterpRatios is None
    again = g.parameterize(_cuda(pts), _cuda(nm) if with_normals else None,
                           _cuda(cl))
    assert torch.equal(again.Grid8NbIndices, got.Grid8NbIndices)
    _same(again.Grid8NbVertexInterpRatios, got.Grid8NbVertexInterpRatios,
          "second run")
    _same(again.positions, got.positions, "second run positions")


def test_parameterize_with_normals():
    _check_parameterize(True)


def test_parameterize_without_normals():
    _check_parameterize(False)


# ---- deform (cloud) ---------------------------------------------------------

def test_deform_cloud_through_a_displaced_grid():
    p, nm, cl = _cloud()
    g = _touched(p)
    _displace(g)
    grid = _grid_dict(g)
    want = co.parameterize(p, GRID, grid, nm)
    corners = co.corner_positions(want["keys"], grid)
    want_pos, want_nrm = co.deform(corners, want["vertex"], want["normal"])
    assert np.abs(want_pos - p).max() > 1e-3, "the grid must move the points"
    cloud = g.parameterize(_cuda(p), _cuda(nm), _cuda(cl))
    pos, nrm, colors = g.deform(cloud)
    _same(pos, want_pos, "deformed positions")
    _same(nrm, want_nrm, "deformed normals")
    _same(colors, cl, "colors pass through")
    pos2, nrm2, _ = g.deform(cloud)
    _same(pos2, pos, "second run")
    _same(nrm2, nrm, "second run normals")


def test_deform_refuses_indices_out_of_range():
    p, nm, cl = _cloud()
    g = _touched(p)
    cloud = g.parameterize(_cuda(p), _cuda(nm))
    cap = g.get_hashmap().capacity()
    for bad in (cap, -1, 2 ** 31 - 1):
        idx = cloud.Grid8NbIndices.clone()
        idx[len(idx) // 2, 5] = bad
        cloud_bad = type(cloud)(cloud.positions, cloud.normals, None, idx,
                                cloud.Grid8NbVertexInterpRatios,
                                cloud.Grid8NbNormalInterpRatios)
        out_p = torch.full((len(idx), 3), 7.5, device="cuda")
        out_n = torch.full((len(idx), 3), -2.5, device="cuda")
        assert g.deform_raw(cloud_bad, out_p, out_n) == INVALID_ARG
        assert (out_p == 7.5).all() and (out_n == -2.5).all()


# ---- project ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _project_case():
    from open3d_amd import synthetic as syn
    rng = np.random.RandomState(17)
    K = syn.intrinsics(W, H)
    T = syn.pose(40)
    n = 3000
    z = rng.uniform(0.4, 3.6, n)  # some beyond depth_max
    u = rng.uniform(-12, W + 12, n)  # some outside the image
    v = rng.uniform(-12, H + 12, n)
    cam = np.stack([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1],
                    z, np.ones(n)], 1)
    world = (np.linalg.inv(T) @ cam.T).T[:, :3].astype(F)
    world[5] = [np.nan, 0, 1]
    # exact duplicates further down: equal d, the lower index must win
    world = np.concatenate([world, world[100:400]])
    colors = rng.uniform(0, 1, (len(world), 3)).astype(F)
    return world, colors, K, T


def test_project_to_images():
    from open3d_amd import slac
    world, colors, K, T = _project_case()
    want_d, want_c, hits = co.project(world, K, T, H, W, SCALE, DMAX, colors,
                                      return_hits=True)
    assert np.count_nonzero(hits >= 2) >= 20
    assert hits.sum() < len(world) - 100, "some points must be skipped"
    d, c = slac.project_to_rgbd_image(_cuda(world), _cuda(colors), W, H, K, T,
                                      SCALE, DMAX)
    _same(d, want_d, "depth")
    _same(c, want_c, "color")
    _same(slac.project_to_depth_image(_cuda(world), W, H, K, T, SCALE, DMAX),
          want_d, "depth-only")
    d2, c2 = slac.project_to_rgbd_image(_cuda(world), _cuda(colors), W, H, K,
                                        T, SCALE, DMAX)
    _same(d2, d, "second run")
    _same(c2, c, "second run color")


# ---- deform (images) --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frames():
    depth, color, K, Ts = _scene.frames(0, 3, W, H)
    return depth, color, K, Ts


@functools.lru_cache(maxsize=None)
def _frame_grid(displaced):
    """A grid touched by the clouds of the three frames, and its dict."""
    depth, _, K, Ts = _frames()
    pts = np.concatenate([co.unproject(depth[i], K, Ts[i], SCALE, DMAX)[0]
                          for i in range(3)])
    g = _touched(pts)
    g.compactify()
    if displaced:
        _displace(g)
    return g, _grid_dict(g)


@functools.lru_cache(maxsize=None)
def _oracle_frame(displaced, i):
    depth, color, K, Ts = _frames()
    _, grid = _frame_grid(displaced)
    return co.deform_image(depth[i], color[i], K, Ts[i], SCALE, DMAX, GRID,
                           grid)


@pytest.mark.parametrize("displaced", [False, True])
def test_deform_rgbd_image_fused_chain_and_oracle_agree(displaced):
    depth, color, K, Ts = _frames()
    g, _ = _frame_grid(displaced)
    want_d, want_c = _oracle_frame(displaced, 1)
    d16, c8 = _cuda(depth[1]), _cuda(color[1])
    d, c = g.deform((d16, c8), K, Ts[1], SCALE, DMAX)
    assert d.dtype == torch.float32 and c.dtype == torch.float32
    _same(d, want_d, "fused depth vs oracle")
    _same(c, want_c, "fused color vs oracle")
    cd, cc = g.deform_seam_by_seam(d16, c8, K, Ts[1], SCALE, DMAX)
    _same(cd, d, "chain depth vs fused")
    _same(cc, c, "chain color vs fused")
    _same(g.deform(d16, K, Ts[1], SCALE, DMAX), d, "depth-only fused")
    _same(g.deform_seam_by_seam(d16, None, K, Ts[1], SCALE, DMAX), d,
          "depth-only chain")
    # the Float32 input convention gives the same frame
    df, cf = _scene.as_f32_inputs(depth[1], color[1])
    d_f32, _ = g.deform((_cuda(df), _cuda(co.color_to_float(color[1]))), K,
                        Ts[1], SCALE, DMAX)
    _same(d_f32, d, "float inputs")
    d2, c2 = g.deform((d16, c8), K, Ts[1], SCALE, DMAX)
    _same(d2, d, "second run")
    _same(c2, c, "second run color")


def test_displaced_grid_changes_the_frame():
    plain, _ = _oracle_frame(False, 1)
    moved, _ = _oracle_frame(True, 1)
    valid = (plain > 0) & (moved > 0)
    assert valid.sum() > 0.5 * W * H
    changed = np.count_nonzero(plain[valid] != moved[valid])
    assert changed > 0.1 * valid.sum(), (changed, int(valid.sum()))


def test_create_from_exported_keys_and_values():
    from open3d_amd import slac
    depth, color, K, Ts = _frames()
    g, _ = _frame_grid(True)
    act, keys, curr = _nodes(g)
    h = slac.ControlGrid(GRID, keys=_cuda(keys), values=_cuda(curr))
    assert h.size() == len(keys)
    assert h.get_hashmap().capacity() == 2 * len(keys)
    d16, c8 = _cuda(depth[2]), _cuda(color[2])
    d, c = g.deform((d16, c8), K, Ts[2], SCALE, DMAX)
    hd, hc = h.deform((d16, c8), K, Ts[2], SCALE, DMAX)
    _same(hd, d, "depth")
    _same(hc, c, "color")
    assert np.count_nonzero(d.cpu().numpy()) > 0.5 * W * H


# ---- end to end: the slac_integrate loop ------------------------------------

def _integrate(frames_dc):
    from open3d_amd.geometry import VoxelBlockGrid
    _, _, K, Ts = _frames()
    vbg = VoxelBlockGrid(("tsdf", "weight", "color"),
                         (torch.float32, torch.float32, torch.float32),
                         ((1), (1), (3)), 0.03, 8, 6000)
    for (d, c), T in zip(frames_dc, Ts):
        d, c = d.contiguous(), c.contiguous()
        blocks = vbg.compute_unique_block_coordinates(d, K, T, SCALE, DMAX)
        vbg.integrate(blocks, d, c, K, K, T, SCALE, DMAX)
    hm = vbg.hashmap()
    act = hm.active_buf_indices().long()
    keys = hm.key_tensor()[act].cpu().numpy()
    order = np.lexsort(keys.T[::-1])
    out = [keys[order]]
    for name in ("tsdf", "weight", "color"):
        out.append(vbg.attribute(name)[act].cpu().numpy()[order])
    return out


def test_deformed_integration_matches_the_oracle_frames():
    depth, color, K, Ts = _frames()
    g, _ = _frame_grid(True)
    got = _integrate([g.deform((_cuda(depth[i]), _cuda(color[i])), K, Ts[i],
                               SCALE, DMAX) for i in range(3)])
    want = _integrate([tuple(_cuda(a) for a in _oracle_frame(True, i))
                       for i in range(3)])
    assert len(got[0]) > 50
    assert np.array_equal(got[0], want[0]), "block set"
    for name, a, b in zip(("tsdf", "weight", "color"), got[1:], want[1:]):
        _same(a, b, name)
    assert np.count_nonzero(got[2]) > 1000 and got[3].max() > 0
