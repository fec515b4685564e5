"""GPU parity of the integrate role's per-item code (vbg_stream.hip,
IntegrateRoleWide): the lane -> voxel map, the scalar-base addressing of the
voxel state, the work item's facts taken on the packed uint16 words (c_small,
may_wrap), the packed narrowing at the store, and the round loop over the
rounds that have a frame.

Every case is a small scene (64 x 48 images, a few dozen blocks) integrated in
groups of 1, 4, 5, 12 and 16 frames -- a round (4 frames) boundary falls inside
a group -- and compared bit for bit (tsdf, weight, colour) with the CPU oracle:

  fresh               an empty grid: every pair of voxels starts at weight 0
  pair_weights_differ after 3 frames the odd-x voxels of every other block get
                      5 more weight: the two voxels of those lanes differ from
                      the first frame of the main phase on
  depth_edge          (the scene of every case) a depth step in the middle of
                      the image and blocks that reach over the image border:
                      lanes that update one voxel of their pair and not the
                      other in the middle of a group
  dead_frames         two frames of the main phase are valid in a 16 x 16
                      patch only: blocks they touch carry their bit, but most
                      waves update nothing in them, between frames that do
  weight_near_wrap    weights pre-loaded at 65530: may_wrap sends the items to
                      the general copy and the uint16 weights wrap
  colour_above_255    a c_small that is wrongly true must change the result.
                      The short copy differs from the general one only in
                      fma(weight, c, in) against weight * c + in, and their
                      truncated means differ only where the mean sits on an
                      integer: the case's images have ONE colour (77), every
                      third block gets weights w of 30000-30006 and, in one of
                      the six uint16 positions of a lane's colour words (3
                      channels x the pair's 2 voxels, one position per block),
                      colours of w + 78 (+-1) -- about 0x7580, a value above
                      255 in either byte order of the test -- so that
                      (w c + 77) / (w + 1) is c - 1 to within the rounding of
                      w c (near 2^30, one unit = 64). Replayed in numpy, the
                      two forms part in 19 % of such voxels at the first
                      update and in 76 % after eight; run against a build
                      whose mask misses the upper halfwords, every block
                      edited in an upper halfword comes out different (757,
                      1333, 24 and 199 colour values in the four of them) and
                      all five group sizes of the case fail
  res8 / res4 / res12 8^3 blocks (the cube map with no high x bit), 4^3 blocks
                      (the slab map) and 12^3 blocks (no power of two: the
                      dividing map). The library offers no switch that turns
                      the cube map off at 16^3, so "cube off" is covered
                      through these two resolutions only."""
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
N_PRE, N_MAIN = 3, 16
N = N_PRE + N_MAIN
GROUPS = (1, 4, 5, 12, 16)
CASES = ("fresh", "pair_weights_differ", "depth_edge", "dead_frames",
         "weight_near_wrap", "colour_above_255", "res8", "res4", "res12")
COLOUR_IN = 77  # colour_above_255: the one colour of its images
DEAD = (N_PRE + 6, N_PRE + 9)  # dead_frames: inside every group longer than 1
# power-of-two focal length: the prepare tables are the identity
K = np.array([[64.0, 0, 31.5], [0, 64.0, 23.5], [0, 0, 1]])


def _res(case):
    return {"res8": 8, "res4": 4, "res12": 12}.get(case, 16)


def _capacity(case):
    return 4096 if case == "res4" else 512


@functools.lru_cache(maxsize=None)
def _frames(case):
    """Depths (uint16), colours and extrinsics: a wall 0.40 m away with a step
    to 0.52 m at column 36 (more than the truncation distance), seen through a
    window of the image so that the touched blocks reach over its border, by a
    camera that drifts and turns a little from frame to frame."""
    rng = np.random.default_rng(11)
    ds, cs, Ts = [], [], []
    for i in range(N):
        d = np.zeros((H, W), np.uint16)
        d[6:42, 6:36] = 400 + (i % 3)
        d[6:42, 36:58] = 520 - (i % 2)
        d[::11, ::7] = 0
        if case == "dead_frames" and i in DEAD:
            keep = d[8:24, 8:24].copy()
            d[:] = 0
            d[8:24, 8:24] = keep
        ds.append(d)
        c = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        if case == "colour_above_255":
            c[:] = COLOUR_IN
        cs.append(c)
        a = 0.004 * (i + 1)
        T = np.eye(4)
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), \
            np.cos(a)
        T[:3, 3] = (0.0031 * (i + 1), -0.0017 * (i + 1), 0.0011 * (i + 1))
        Ts.append(T)
    return ds, cs, Ts


def _edit_state(case, keys, weight, color):
    """The state edit of a case after the first N_PRE frames, in place on
    block-major numpy arrays ([block, z, y, x]); blocks by sorted key so that
    the oracle and the GPU side pick the same."""
    order = np.lexsort(np.asarray(keys).T[::-1])
    if case == "pair_weights_differ":
        for b in order[::2]:
            weight[b][:, :, 1::2] += 5
    elif case == "weight_near_wrap":
        for b in order[::2]:
            weight[b][:] = 65530
    elif case == "colour_above_255":
        rng = np.random.default_rng(7)
        for j, b in enumerate(order[::3]):
            ch, par = _colour_position(j)
            x = np.arange(par, 16, 2)
            w = np.broadcast_to(30000 + np.arange(16) % 7, (16, 16, 16))
            weight[b][:] = w.astype(np.uint16)
            jitter = rng.integers(-1, 2, (16, 16, x.size))
            color[b][:, :, x, ch] = (w[:, :, x] + 1 + COLOUR_IN +
                                     jitter).astype(np.uint16)


def _colour_position(j):
    """(channel, x parity) of the j-th edited block of colour_above_255: the
    six uint16 positions of a lane's three colour words in turn"""
    return j % 3, (j // 3) % 2


@functools.lru_cache(maxsize=None)
def _oracle_run(case):
    ds, cs, Ts = _frames(case)
    res, cap = _res(case), _capacity(case)
    trunc = sc.VOXEL * sc.TRUNC_MULT
    h = orc.HashMap(cap)
    tsdf = np.zeros((cap, res, res, res), np.float32)
    wgt = np.zeros((cap, res, res, res), np.uint16)
    col = np.zeros((cap, res, res, res, 3), np.uint16)
    for i in range(N):
        if i == N_PRE:
            n = h.size()
            keys = h.key_buffer()[:n].copy()
            buf, _ = h.find(keys)
            w, c = wgt[buf], col[buf]
            _edit_state(case, keys, w, c)
            wgt[buf], col[buf] = w, c
        keys = orc.depth_touch(ds[i], K, Ts[i], res, sc.VOXEL, trunc,
                               sc.DEPTH_SCALE, sc.DEPTH_MAX, 4)
        assert len(keys) > 0
        h.activate(keys)
        buf, m = h.find(keys)
        assert m.all()
        orc.integrate(ds[i], cs[i], buf, h.key_buffer(), tsdf, wgt, col, K, K,
                      Ts[i], res, sc.VOXEL, trunc, sc.DEPTH_SCALE,
                      sc.DEPTH_MAX)
    n = h.size()
    keys = h.key_buffer()[:n].copy()
    buf, _ = h.find(keys)
    return _sorted((keys, tsdf[buf], wgt[buf], col[buf]))


def _gpu_run(case, group):
    from open3d_amd import _lib, geometry
    L = _lib.lib()
    # launches take the IEEE forms until the on-device proof of the short
    # divisions is over: wait for it, so that the short forms run here
    assert L.o3dmi_vbg_division_forms(C.c_float(sc.VOXEL),
                                      C.c_float(sc.TRUNC_MULT), 1) == 2
    ds, cs, Ts = _frames(case)
    g = geometry.VoxelBlockGrid(["tsdf", "weight", "color"],
                                [torch.float32, torch.uint16, torch.uint16],
                                [1, 1, 3], voxel_size=sc.VOXEL,
                                block_resolution=_res(case),
                                block_count=_capacity(case))
    dt = [torch.from_numpy(d).cuda() for d in ds]
    ct = [torch.from_numpy(c).cuda() for c in cs]

    def integrate(lo, hi):
        g.integrate_frames(dt[lo:hi], ct[lo:hi], K, K, Ts[lo:hi],
                           sc.DEPTH_SCALE, sc.DEPTH_MAX, sc.TRUNC_MULT,
                           frames_per_launch=group)

    def state():
        hm = g.hashmap()
        idx = hm.active_buf_indices()
        keys = hm.key_tensor().cpu().numpy()[idx.cpu().numpy()]
        return keys, idx.long()

    def forms():
        return [int(L.o3dmi_vbg_step_form_launches(f)) for f in range(3)]

    before = forms()
    integrate(0, N_PRE)
    torch.cuda.synchronize()
    keys, i64 = state()
    # uint16 state edited through an int16 view of the same bytes
    wv = g.attribute("weight").view(torch.int16)
    cv = g.attribute("color").view(torch.int16)
    w = wv[i64].cpu().numpy().view(np.uint16)[..., 0].copy()
    c = cv[i64].cpu().numpy().view(np.uint16).copy()
    _edit_state(case, keys, w, c)
    wv[i64] = torch.from_numpy(w.view(np.int16)[..., None]).cuda()
    cv[i64] = torch.from_numpy(c.view(np.int16)).cuda()
    integrate(N_PRE, N)
    torch.cuda.synchronize()
    ieee_launches = forms()[0] - before[0]
    keys, i64 = state()
    t = g.attribute("tsdf")[i64].cpu().numpy()[..., 0]
    w = g.attribute("weight").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16)[..., 0]
    c = g.attribute("color").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16)
    return _sorted((keys, t, w, c)), ieee_launches


def _sorted(run):
    keys, t, w, c = run
    o = np.lexsort(np.asarray(keys).T[::-1])
    return (np.asarray(keys)[o], np.ascontiguousarray(t[o]),
            np.ascontiguousarray(w[o]), np.ascontiguousarray(c[o]))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("case", CASES)
def test_per_item_code_equals_oracle(case, group):
    (ks, ts, ws, cs), ieee_launches = _gpu_run(case, group)
    kw, tw, ww, cw = _oracle_run(case)
    # the short-division forms ran (the kernels whose per-item code this is)
    assert ieee_launches == 0
    assert np.array_equal(ks, kw)
    assert np.array_equal(ws, ww)
    assert np.array_equal(cs, cw)
    assert ts.tobytes() == tw.tobytes()
    # the case is what it says
    assert 8 <= len(ks) <= _capacity(case) // 2
    if case == "fresh":
        # lanes whose two voxels ended at different weights: a pair parted
        assert (ws[..., 0::2] != ws[..., 1::2]).any()
        assert (ws == N).any()
    elif case == "weight_near_wrap":
        assert (ws < 100).any() and (ws > 65500).any()  # wrapped and not
    elif case == "colour_above_255":
        assert (cs > 30000).any() and ((ws > 30006) & (ws < 30007 + N)).any()
    elif case == "dead_frames":
        assert (ws == N - len(DEAD)).any()
