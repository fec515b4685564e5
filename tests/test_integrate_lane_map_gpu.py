"""GPU parity of the integrate role's lane -> voxel map (vbg_stream.hip,
IntegrateRoleWide): on the cube path a lane owns the voxels r and r + 4 of its
wave's 8-voxel x-run, while the state keeps its layout in memory -- a lane
loads and stores a contiguous pair and trades one value of each pair with the
lane two further on in its quad (QuadTrade), after the load and before the
store. The slab path (resolutions below 8, or no power of two) trades nothing.

Every case is a small stream (64 x 48 images, a wall with a depth step seen
through a window that reaches the image's left border, so that blocks straddle
the border and lanes of both slots read the sentinel record), integrated in
groups of 1, 4, 5 and 12 frames -- one round, a full round, a partial second
round, three rounds -- and compared bit for bit (tsdf, weight, colour) with the
CPU oracle. After the first two frames the state of every block is overwritten
with values that are functions of the voxel's linear index, distinct in every
voxel of a block, and two frames of the main phase are valid in the left half
of the image only: lanes whose voxels those frames do not update sit beside
lanes they do. A trade that puts a value into the wrong lane or slot, or a
store-side trade that is not the load-side one's inverse, moves distinct values
and cannot cancel out.

  res 16, 8     the cube path (8: its smallest form, one cube per wave in x)
  res 4, 6      the slab path (6: no power of two)
  u16 / f32     grid types, each with and without colour
  colour_above_255, weight_near_wrap
                the edited state has colours above 255 / weights within a
                group of 65535: the work item takes the general copy"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _oracle as orc  # noqa: E402
import _scene as sc  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
N_PRE, N_MAIN = 2, 12
N = N_PRE + N_MAIN
GROUPS = (1, 4, 5, 12)
HALF = (N_PRE + 1, N_PRE + 6)  # frames valid in the left half only
# power-of-two focal length: the prepare tables are the identity
K = np.array([[64.0, 0, 31.5], [0, 64.0, 23.5], [0, 0, 1]])

# case -> (resolution, grid is float32, with colour, state edit)
CASES = {
    "u16_colour_res16": (16, False, True, "index"),
    "u16_colour_res8": (8, False, True, "index"),
    "u16_colour_res4": (4, False, True, "index"),
    "u16_colour_res6": (6, False, True, "index"),
    "u16_plain_res16": (16, False, False, "index"),
    "f32_colour_res16": (16, True, True, "index"),
    "f32_colour_res8": (8, True, True, "index"),
    "f32_plain_res16": (16, True, False, "index"),
    "colour_above_255": (16, False, True, "colour_above_255"),
    "weight_near_wrap": (16, False, True, "weight_near_wrap"),
}


def _capacity(res):
    return 4096 if res < 8 else 512


@functools.lru_cache(maxsize=None)
def _frames():
    rng = np.random.default_rng(12)
    ds, cs, Ts = [], [], []
    for i in range(N):
        d = np.zeros((H, W), np.uint16)
        d[4:44, 0:36] = 400 + (i % 3)
        d[4:44, 36:58] = 520 - (i % 2)
        d[::11, ::7] = 0
        if i in HALF:
            d[:, W // 2:] = 0
        ds.append(d)
        cs.append(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
        a = 0.004 * (i + 1)
        T = np.eye(4)
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), \
            np.cos(a)
        T[:3, 3] = (0.0031 * (i + 1), -0.0017 * (i + 1), 0.0011 * (i + 1))
        Ts.append(T)
    return ds, cs, Ts


def _edit_state(edit, tsdf, weight, color):
    """In place on block-major arrays ([block, z, y, x(, channel)]): every
    value a function of the voxel's linear index in its block."""
    res = tsdf.shape[1]
    lin = np.arange(res ** 3).reshape(res, res, res)
    tsdf[:] = (lin / np.float32(res ** 3) - np.float32(0.5)).astype(np.float32)
    weight[:] = (lin + 10).astype(weight.dtype)
    if edit == "weight_near_wrap":
        weight[:] = (65535 - 6 - lin % 5).astype(weight.dtype)
    if color is not None:
        for ch in range(3):
            color[..., ch] = ((lin * 5 + 83 * ch) % 256).astype(color.dtype)
        if edit == "colour_above_255":
            color[..., 1] = (300 + lin).astype(color.dtype)


@functools.lru_cache(maxsize=None)
def _oracle_run(case):
    res, f32, with_color, edit = CASES[case]
    ds, cs, Ts = _frames()
    cap = _capacity(res)
    st = np.float32 if f32 else np.uint16
    trunc = sc.VOXEL * sc.TRUNC_MULT
    h = orc.HashMap(cap)
    tsdf = np.zeros((cap, res, res, res), np.float32)
    wgt = np.zeros((cap, res, res, res), st)
    col = np.zeros((cap, res, res, res, 3), st) if with_color else None
    for i in range(N):
        if i == N_PRE:
            buf, _ = h.find(h.key_buffer()[:h.size()].copy())
            t, w = tsdf[buf], wgt[buf]
            c = col[buf] if with_color else None
            _edit_state(edit, t, w, c)
            tsdf[buf], wgt[buf] = t, w
            if with_color:
                col[buf] = c
        keys = orc.depth_touch(ds[i], K, Ts[i], res, sc.VOXEL, trunc,
                               sc.DEPTH_SCALE, sc.DEPTH_MAX, 4)
        assert len(keys) > 0
        h.activate(keys)
        buf, m = h.find(keys)
        assert m.all()
        orc.integrate(ds[i], cs[i] if with_color else None, buf,
                      h.key_buffer(), tsdf, wgt, col, K, K, Ts[i], res,
                      sc.VOXEL, trunc, sc.DEPTH_SCALE, sc.DEPTH_MAX)
    keys = h.key_buffer()[:h.size()].copy()
    buf, _ = h.find(keys)
    return _sorted((keys, tsdf[buf], wgt[buf],
                    col[buf] if with_color else None))


def _sorted(run):
    keys, t, w, c = run
    o = np.lexsort(np.asarray(keys).T[::-1])
    return (np.asarray(keys)[o], np.ascontiguousarray(t[o]),
            np.ascontiguousarray(w[o]),
            np.ascontiguousarray(c[o]) if c is not None else None)


def _gpu_run(case, group):
    from open3d_amd import _lib, geometry
    L = _lib.lib()
    # launches take the IEEE forms until the on-device proof of the short
    # divisions is over: wait for it, so that the short forms run here
    assert L.o3dmi_vbg_division_forms(C.c_float(sc.VOXEL),
                                      C.c_float(sc.TRUNC_MULT), 1) == 2
    res, f32, with_color, edit = CASES[case]
    ds, cs, Ts = _frames()
    st = torch.float32 if f32 else torch.uint16
    names = ["tsdf", "weight"] + (["color"] if with_color else [])
    g = geometry.VoxelBlockGrid(names, [torch.float32, st] +
                                ([st] if with_color else []),
                                [1, 1] + ([3] if with_color else []),
                                voxel_size=sc.VOXEL, block_resolution=res,
                                block_count=_capacity(res))
    dt = [torch.from_numpy(d).cuda() for d in ds]
    ct = [torch.from_numpy(c).cuda() for c in cs] if with_color else None

    def integrate(lo, hi):
        g.integrate_frames(dt[lo:hi], ct[lo:hi] if ct else None, K, K,
                           Ts[lo:hi], sc.DEPTH_SCALE, sc.DEPTH_MAX,
                           sc.TRUNC_MULT, frames_per_launch=group)

    def view(name):
        # uint16 state goes through an int16 view of the same bytes
        a = g.attribute(name)
        return a if f32 else a.view(torch.int16)

    def fetch(name, i64):
        a = view(name)[i64].cpu().numpy()
        return a if f32 else a.view(np.uint16)

    def rows():
        hm = g.hashmap()
        idx = hm.active_buf_indices()
        return hm.key_tensor().cpu().numpy()[idx.cpu().numpy()], idx.long()

    integrate(0, N_PRE)
    torch.cuda.synchronize()
    _, i64 = rows()
    t = g.attribute("tsdf")[i64].cpu().numpy()[..., 0].copy()
    w = fetch("weight", i64)[..., 0].copy()
    c = fetch("color", i64).copy() if with_color else None
    _edit_state(edit, t, w, c)
    put = (lambda a: a) if f32 else (lambda a: a.view(np.int16))
    g.attribute("tsdf")[i64] = torch.from_numpy(t[..., None]).cuda()
    view("weight")[i64] = torch.from_numpy(put(w)[..., None]).cuda()
    if with_color:
        view("color")[i64] = torch.from_numpy(put(c)).cuda()
    integrate(N_PRE, N)
    torch.cuda.synchronize()
    keys, i64 = rows()
    return _sorted((keys, g.attribute("tsdf")[i64].cpu().numpy()[..., 0],
                    fetch("weight", i64)[..., 0],
                    fetch("color", i64) if with_color else None))


def _outside_by_slot(res):
    """Voxels of the first main frame's blocks that project outside the image,
    counted per slot of the cube path's lanes (x % 8 < 4 / >= 4)."""
    ds, _, Ts = _frames()
    i = N_PRE
    keys = np.asarray(orc.depth_touch(ds[i], K, Ts[i], res, sc.VOXEL,
                                      sc.VOXEL * sc.TRUNC_MULT, sc.DEPTH_SCALE,
                                      sc.DEPTH_MAX, 4))
    g = np.arange(res)
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    loc = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    p = (keys[:, None, :] * res + loc[None]) * sc.VOXEL
    pc = p @ Ts[i][:3, :3].T + Ts[i][:3, 3]
    u = K[0, 0] * pc[..., 0] / pc[..., 2] + K[0, 2]
    v = K[1, 1] * pc[..., 1] / pc[..., 2] + K[1, 2]
    out = (pc[..., 2] > 0) & ~((u >= 0) & (u <= W - 1) & (v >= 0) &
                               (v <= H - 1))
    slot = np.broadcast_to(loc[:, 0] % 8 >= 4, out.shape)
    return int((out & ~slot).sum()), int((out & slot).sum())


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("case", list(CASES))
def test_lane_map_equals_oracle(case, group):
    res, f32, with_color, edit = CASES[case]
    ks, ts, ws, cs = _gpu_run(case, group)
    kw, tw, ww, cw = _oracle_run(case)
    assert np.array_equal(ks, kw)
    assert ws.tobytes() == ww.tobytes()
    if with_color:
        assert cs.tobytes() == cw.tobytes()
    else:
        assert cs is None
    assert ts.tobytes() == tw.tobytes()
    # the case is what it says: some voxels took every frame of the main
    # phase, some none (their edited state came through the trades untouched)
    assert 8 <= len(ks) <= _capacity(res) // 2
    lin = np.arange(res ** 3).reshape(res, res, res)
    if edit == "weight_near_wrap":
        assert (ws < 100).any() and (ws > 65500).any()  # wrapped and not
    else:
        grown = ws.astype(np.int64) - (lin + 10)
        assert (grown == N_MAIN).any() and (grown == 0).any()
        assert (grown == N_MAIN - len(HALF)).any()
    if edit == "colour_above_255":
        assert (cs > 255).any()


def test_blocks_straddle_the_image_border_in_both_slots():
    lo, hi = _outside_by_slot(16)
    assert lo > 0 and hi > 0, (lo, hi)
