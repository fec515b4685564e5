"""Ray-cast test cases that need no GPU to build: the oracle-side grid and the
recipes (size, pose, intrinsics, depth limits) that put RayCastKernel into
each of its launch forms, beyond the LDS block table's reach, and at poses
that were never integrated.

One grid serves every case of a block resolution: frames 300, 302, 304 and
306 of the synthetic room at 320 x 240. The ray-cast size is independent of
the integrated size; the pose recipe is

    T = Ry(yaw) @ T_last;  T[0, 3] += shift;  T[2, 3] += back

with T_last the world-to-camera pose of frame 306 (`back` moves the camera
straight backwards along its own axis), and `zoom` multiplies the focal
lengths.

A workgroup tile is 32 x 8 pixels; the form is chosen from the tile count
with 256 CUs (test_extension_loaded_and_device pins that number):
    <= 1280 tiles        bands
    1281 .. 4096 tiles   rounds (one workgroup per tile)
    > 4096 tiles         strided (4096 workgroups loop over the tiles)
"""
import collections
import functools
import math

import numpy as np

import _oracle as orc
import _scene as sc
from open3d_amd import synthetic

FRAMES = (300, 302, 304, 306)
FRAME_W, FRAME_H = 320, 240
DEPTH_MIN = 0.1
WEIGHT_THRESHOLD = 1.0
DOWN = 8
CUS = 256  # kCUs; pinned by test_vbg_gpu.test_extension_loaded_and_device
ALL_ATTRS = ("depth", "vertex", "color", "normal", "index", "mask",
             "interp_ratio", "interp_ratio_dx", "interp_ratio_dy",
             "interp_ratio_dz")
MAPS = ("depth", "vertex", "normal", "color")


class OracleGrid:
    """Oracle-side VoxelBlockGrid: hash + numpy value buffers."""

    def __init__(self, grid_f32, capacity, with_color=True, res=sc.RES):
        self.h = orc.HashMap(capacity)
        wd = np.float32 if grid_f32 else np.uint16
        self.res = res
        self.tsdf = np.zeros((capacity, res, res, res), np.float32)
        self.weight = np.zeros((capacity, res, res, res), wd)
        self.color = np.zeros((capacity, res, res, res, 3), wd) \
            if with_color else None

    def integrate(self, depth, color, K, T, keys=None):
        if keys is None:
            keys = orc.depth_touch(depth, K, T, self.res, sc.VOXEL,
                                   sc.VOXEL * sc.TRUNC_MULT, sc.DEPTH_SCALE,
                                   sc.DEPTH_MAX, 4)
        self.h.activate(keys)
        buf, m = self.h.find(keys)
        assert m.all()
        orc.integrate(depth, color, buf, self.h.key_buffer(), self.tsdf,
                      self.weight, self.color, K, K, T, self.res, sc.VOXEL,
                      sc.VOXEL * sc.TRUNC_MULT, sc.DEPTH_SCALE, sc.DEPTH_MAX)
        return keys


# name -> (res, w, h, yaw, shift, back, zoom, depth_max)
RECIPES = {
    "rounds": (16, 1304, 264, 0.0, 0.0, 0.0, 1.0, 3.0),
    "strided": (16, 1304, 808, 0.0, 0.0, 0.0, 1.0, 3.0),
    "novel_a": (16, 320, 240, 0.25, 0.15, 0.0, 1.0, 3.0),
    "novel_b": (16, 320, 240, -0.4, -0.3, 0.0, 1.0, 3.0),
    "novel_c": (16, 320, 240, 0.6, 0.0, 0.3, 1.0, 3.0),
    "far": (8, 160, 120, 0.0, 0.0, 6.5, 4.0, 12.0),
    # `far` leaves the block table's reach on +x only. The table's tag is
    # three offsets biased by 128 and held as UNSIGNED: past +127 they
    # overflow upwards, below -128 they wrap to 0xFFFFFFxx, and only the
    # wrapped y and z spill over the other axes' bits. This view has its hit
    # blocks 98 to 138 blocks away on -z.
    "far_neg": (8, 160, 120, -0.45, 0.5, 8.7, 4.0, 12.0),
}
GRID_CAPACITY = {16: 4096, 8: 16384}

Case = collections.namedtuple(
    "Case", "name og keys K T w h depth_min depth_max res frame_keys")


def tile_count(w, h):
    return ((w + 31) // 32) * ((h + 7) // 8)


def launch_form(w, h):
    n = tile_count(w, h)
    return "bands" if n <= CUS * 5 else ("rounds" if n <= CUS * 16
                                         else "strided")


def novel_pose(T_last, yaw=0.0, shift=0.0, back=0.0):
    c, s = math.cos(yaw), math.sin(yaw)
    Ry = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]],
                  np.float64)
    T = Ry @ np.asarray(T_last, np.float64)
    T[0, 3] += shift
    T[2, 3] += back
    return T


@functools.lru_cache(maxsize=None)
def grid(res, grid_f32):
    """-> (OracleGrid, keys, per-frame key sets, T_last): the four frames
    integrated; `keys` is the row-unique union of their depth_touch sets.
    Shared between the tests: nobody writes to it."""
    og = OracleGrid(grid_f32, GRID_CAPACITY[res], res=res)
    per_frame = []
    for k in FRAMES:
        d, c, K, Ts = sc.frames(k, 1, FRAME_W, FRAME_H)
        per_frame.append(og.integrate(d[0], c[0], K, Ts[0]))
    keys = np.ascontiguousarray(np.unique(np.concatenate(per_frame), axis=0))
    return og, keys, tuple(per_frame), Ts[0]


def case(name, grid_f32=False):
    res, w, h, yaw, shift, back, zoom, depth_max = RECIPES[name]
    og, keys, per_frame, T_last = grid(res, bool(grid_f32))
    K = synthetic.intrinsics(w, h)
    K[0, 0] *= zoom
    K[1, 1] *= zoom
    return Case(name, og, keys, K, novel_pose(T_last, yaw, shift, back), w, h,
                DEPTH_MIN, depth_max, res, per_frame)


def rounds(grid_f32=False):
    return case("rounds", grid_f32)


def strided(grid_f32=False):
    return case("strided", grid_f32)


def novel_a(grid_f32=False):
    return case("novel_a", grid_f32)


def novel_b(grid_f32=False):
    return case("novel_b", grid_f32)


def novel_c(grid_f32=False):
    return case("novel_c", grid_f32)


def far(grid_f32=False):
    return case("far", grid_f32)


def far_neg(grid_f32=False):
    return case("far_neg", grid_f32)


def oracle_range(cs, keys=None, T=None, depth_min=None, depth_max=None):
    cap = 1 << 20
    rng, needed = orc.estimate_range(
        cs.keys if keys is None else keys, cs.K, cs.T if T is None else T,
        cs.h, cs.w, DOWN, cs.res, sc.VOXEL,
        cs.depth_min if depth_min is None else depth_min,
        cs.depth_max if depth_max is None else depth_max,
        frag_buffer_size=cap)
    assert needed < cap
    return rng


@functools.lru_cache(maxsize=None)
def oracle_maps(name, grid_f32=False, attrs=MAPS):
    """-> (range map, {attr: map}) of the oracle for a case; rendered once
    and shared (treat as read-only)."""
    cs = case(name, grid_f32)
    rng = oracle_range(cs)
    want = orc.raycast(cs.og.h, cs.og.tsdf, cs.og.weight, cs.og.color, rng,
                       cs.K, cs.T, cs.h, cs.w, cs.res, sc.VOXEL,
                       sc.DEPTH_SCALE, cs.depth_min, cs.depth_max,
                       WEIGHT_THRESHOLD, sc.TRUNC_MULT, DOWN, attrs)
    return rng, want


def block_offsets(cs, vertex, hit):
    """Per hit pixel {n, 3}: the signed offset, in blocks, of the block of
    the world point from the camera's own block (the origin of the ray
    cast's LDS block table, which holds offsets in [-128, 128))."""
    c2w = np.linalg.inv(cs.T)
    block = np.float32(sc.VOXEL) * np.float32(cs.res)
    cam = np.floor(c2w[:3, 3].astype(np.float32) / block).astype(np.int64)
    pw = vertex[hit].astype(np.float64) @ c2w[:3, :3].T + c2w[:3, 3]
    pb = np.floor(pw.astype(np.float32) / block).astype(np.int64)
    return pb - cam


def block_distance(cs, vertex, hit):
    """Per hit pixel: the largest per-axis distance in blocks."""
    return np.abs(block_offsets(cs, vertex, hit)).max(axis=1)
