"""GPU parity of the frame stream's group touch (vbg_stream.hip, TouchRole): one
touch workgroup per 16 x 16 tile of rays collects the block keys of ALL the
frames of a launch in one LDS set {key -> frame bits}, sends each distinct key
through the block hash once, and flushes the set early when the frames could
collect more keys than it holds (o3dmi_vbg_front_tile_key_limit).

Every case integrates small frames (64 x 48 at stride 4: one partial 16 x 12
tile) through integrate_frames and compares the block key set and TSDF, weight
and colour per block key with the CPU oracle, bit for bit. The frame bits are
checked through the launch profile: per launch, the blocks the touch listed
must number the union of the oracle's per-frame key sets, and the block-frames
the integrate role applied (the set bits of all touch words) their sum. (These
are totals per launch; a bit set on the wrong block of a launch would leave
them unchanged, and is caught by the voxel comparison instead.)

  coherent      13 scene frames, frames_per_launch = 12: a full group and a
                1-frame group; the set never flushes early
  two_tiles     the same at 72 x 40: two tiles, both partial
  colourless    coherent, on a grid without colour
  scattered     per-frame random depths over the whole valid range, even
                frames on the upper 8 ray rows only: the keys the tile collects
                over the group pass the limit more than twice, and a flush
                holds more keys than one flush pass hands out (1024)
  all_distinct  one random depth image seen from poses a whole number of
                blocks apart: no key is shared between frames, early flushes
  empty_frame   9 scene frames in groups of 4, frames 2 and 4 with all-zero
                depth: an empty frame inside a group and one that opens a group
  group_sizes   17 scene frames with frames_per_launch = 1, 2 and 16"""
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
# Two figures restate the kernel (vbg_stream.hip) and must follow it: a frame
# adds at most 4 candidates per ray of the tile (TouchRole frame_max; the tile
# here has 16 x 12 rays), and one flush pass hands out kTileDense keys -- if
# that constant changes, the scattered case's "a flush holds more than one
# pass" precondition has to change with it.
FRAME_KEYS = 4 * 16 * 12
DENSE = 1024


@functools.lru_cache(maxsize=None)
def _scene(n, w, h):
    ds, cs, Ts, K = [], [], [], None
    for k in range(200, 200 + 10 * n, 10):
        d, c, K, T = sc.frames(k, 1, w, h)
        ds.append(d[0]); cs.append(c[0]); Ts.append(np.array(T[0], np.float64))
    return ds, cs, K, Ts


def _shifted(T, blocks, res):
    """The extrinsic of the same camera moved by `blocks` blocks along x."""
    S = np.eye(4)
    S[0, 3] = -blocks * res * sc.VOXEL
    return T @ S


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """depths, colours (or None), K, extrinsics, block resolution, capacity"""
    if name in ("coherent", "colourless"):
        ds, cs, K, Ts = _scene(13, W, H)
        return ds, (None if name == "colourless" else cs), K, Ts, 16, 4096
    if name == "two_tiles":
        ds, cs, K, Ts = _scene(13, 72, 40)
        return ds, cs, K, Ts, 16, 4096
    if name == "seventeen":
        ds, cs, K, Ts = _scene(17, W, H)
        return ds, cs, K, Ts, 16, 4096
    if name == "empty_frame":
        ds, cs, K, Ts = _scene(9, W, H)
        ds = list(ds)
        for f in (2, 4):
            ds[f] = np.zeros_like(ds[f])
        return ds, cs, K, Ts, 16, 4096
    rng = np.random.default_rng(11)
    _, cs, K, Ts = _scene(13, W, H)
    raw_max = int(sc.DEPTH_MAX * sc.DEPTH_SCALE)
    if name == "scattered":
        ds = []
        for f in range(13):
            d = rng.integers(1, raw_max, (H, W)).astype(np.uint16)
            if f % 2 == 0:
                d[32:] = 0  # ray rows 8..11 see nothing
            ds.append(d)
        return ds, cs, K, Ts, 8, 16384
    if name == "all_distinct":
        d = rng.integers(1, raw_max, (H, W)).astype(np.uint16)
        return ([d] * 13, cs, K, [_shifted(Ts[0], 128 * f, 8) for f in range(13)],
                8, 16384)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """-> (keys, tsdf, weight, colour) in key order, per-frame key arrays"""
    ds, cs, K, Ts, res, cap = _inputs(name)
    trunc = sc.VOXEL * sc.TRUNC_MULT
    h = orc.HashMap(cap)
    tsdf = np.zeros((cap, res, res, res), np.float32)
    wgt = np.zeros((cap, res, res, res), np.uint16)
    col = np.zeros((cap, res, res, res, 3), np.uint16) if cs else None
    frame_keys = []
    for i in range(len(ds)):
        keys = orc.depth_touch(ds[i], K, Ts[i], res, sc.VOXEL, trunc,
                               sc.DEPTH_SCALE, sc.DEPTH_MAX, 4)
        frame_keys.append(keys)
        if len(keys) == 0:
            continue
        h.activate(keys)
        buf, m = h.find(keys)
        assert m.all()
        orc.integrate(ds[i], cs[i] if cs else None, buf, h.key_buffer(), tsdf,
                      wgt, col, K, K, Ts[i], res, sc.VOXEL, trunc,
                      sc.DEPTH_SCALE, sc.DEPTH_MAX)
    n = h.size()
    keys = h.key_buffer()[:n].copy()
    buf, _ = h.find(keys)
    return _sorted((keys, tsdf[buf], wgt[buf], col[buf] if cs else None)), \
        frame_keys


def _sorted(run):
    keys, t, w, c = run
    o = np.lexsort(np.asarray(keys).T[::-1])
    return (np.asarray(keys)[o], np.ascontiguousarray(t[o]),
            np.ascontiguousarray(w[o]),
            np.ascontiguousarray(c[o]) if c is not None else None)


def _key_limit():
    from open3d_amd import _lib
    limit = int(_lib.lib().o3dmi_vbg_front_tile_key_limit())
    assert 4 * 16 * 16 <= limit < 2048
    return limit


def _flush_sizes(frame_keys, limit):
    """Keys held at every early flush of a group's single tile: the set is
    flushed before a frame that could take it past the limit."""
    held, sizes = set(), []
    for f, keys in enumerate(frame_keys):
        if f > 0 and len(held) + FRAME_KEYS > limit:
            sizes.append(len(held))
            held = set()
        held |= set(map(tuple, keys))
    return sizes


def _gpu_run(name, group):
    from open3d_amd import _lib, geometry
    L = _lib.lib()
    assert L.o3dmi_vbg_division_forms(C.c_float(sc.VOXEL),
                                      C.c_float(sc.TRUNC_MULT), 1) == 2
    ds, cs, K, Ts, res, cap = _inputs(name)
    names = ["tsdf", "weight"] + (["color"] if cs else [])
    dtypes = [torch.float32, torch.uint16] + ([torch.uint16] if cs else [])
    g = geometry.VoxelBlockGrid(names, dtypes, [1, 1] + ([3] if cs else []),
                                voxel_size=sc.VOXEL, block_resolution=res,
                                block_count=cap)
    dt = [torch.from_numpy(d).cuda() for d in ds]
    ct = [torch.from_numpy(c).cuda() for c in cs] if cs else None
    g.profile_begin(64, 1)
    g.integrate_frames(dt, ct, K, K, Ts, sc.DEPTH_SCALE, sc.DEPTH_MAX,
                       sc.TRUNC_MULT, frames_per_launch=group)
    torch.cuda.synchronize()
    g.profile_end()
    prof = g.profile_launches()
    hm = g.hashmap()
    idx = hm.active_buf_indices()
    keys = hm.key_tensor().cpu().numpy()[idx.cpu().numpy()]
    i64 = idx.long()
    t = g.attribute("tsdf")[i64].cpu().numpy()[..., 0]
    w = g.attribute("weight").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16)[..., 0]
    c = g.attribute("color").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16) if cs else None
    return _sorted((keys, t, w, c)), prof


def _check(name, group):
    (kw, tw, ww, cw), frame_keys = _oracle_run(name)
    (ks, ts, ws, cs), prof = _gpu_run(name, group)
    assert np.array_equal(ks, kw)
    assert np.array_equal(ws, ww)
    assert ts.tobytes() == tw.tobytes()
    if cw is None:
        assert cs is None
    else:
        assert np.array_equal(cs, cw)
        assert (cs > 0).any()
    assert (ws > 0).any() and (ws == 0).any()
    # frame bits: blocks listed and block-frames applied, launch by launch
    groups = [frame_keys[f:f + group] for f in range(0, len(frame_keys), group)]
    want_blocks = [len(set(map(tuple, np.concatenate(gk)))) for gk in groups]
    want_bf = [sum(len(k) for k in gk) for gk in groups]
    assert list(prof["distinct_blocks"]) == want_blocks
    assert list(prof["block_frames"]) == want_bf


@pytest.mark.parametrize("name", ["coherent", "two_tiles", "colourless"])
def test_coherent_group_equals_the_oracle(name):
    limit = _key_limit()
    if name != "two_tiles":
        # one tile: the frames' keys are the tile's. No early flush.
        assert _flush_sizes(_oracle_run(name)[1][:12], limit) == []
    _check(name, 12)


def test_scattered_depths_flush_the_set_early():
    limit = _key_limit()
    frame_keys = _oracle_run("scattered")[1]
    full = frame_keys[:12]
    collected = len(set(map(tuple, np.concatenate(full))))
    sizes = _flush_sizes(full, limit)
    # what the case is there for, on its inputs: the group's tile collects
    # more than twice the limit, is flushed early at least twice, and one
    # flush holds more than a flush pass hands out
    assert collected > 2 * limit, (collected, limit)
    assert len(sizes) >= 2 and max(sizes) > DENSE, sizes
    assert all(s <= limit for s in sizes)
    _check("scattered", 12)


def test_frames_without_a_common_key():
    limit = _key_limit()
    frame_keys = _oracle_run("all_distinct")[1]
    sets = [set(map(tuple, k)) for k in frame_keys]
    assert sum(len(s) for s in sets) == len(set().union(*sets))
    assert len(_flush_sizes(frame_keys[:12], limit)) >= 2
    _check("all_distinct", 12)


def test_empty_frames_set_no_bit():
    frame_keys = _oracle_run("empty_frame")[1]
    assert [len(k) == 0 for k in frame_keys] == \
        [f in (2, 4) for f in range(9)]
    _check("empty_frame", 4)


@pytest.mark.parametrize("group", [1, 2, 16])
def test_group_sizes(group):
    _check("seventeen", group)
