"""Poisoned ray casts: every requested output is allocated FILLED -- NaN for
the float maps, 0x77 bytes for `index` and `mask` -- before the C ABI is
called, so a kernel that leaves a pixel unwritten is seen. (torch.empty hands
back the block the previous, often identical, result was just freed from: a
repeated call passes on stale memory whatever the kernel writes.) Misses are
written as zeros, so no poison may be left after a whole-image cast."""
import ctypes as C

import torch

from open3d_amd import _lib
from open3d_amd.core import host_mat, stream

CHANNELS = {"vertex": 3, "normal": 3, "depth": 1, "color": 3, "index": 8,
            "mask": 8, "interp_ratio": 8, "interp_ratio_dx": 8,
            "interp_ratio_dy": 8, "interp_ratio_dz": 8, "range": 2}
_ORDER = ("depth", "vertex", "color", "normal", "index", "mask",
          "interp_ratio", "interp_ratio_dx", "interp_ratio_dy",
          "interp_ratio_dz")
_INDEX_POISON = 0x7777777777777777


def alloc(name, rows, cols):
    shape = (rows, cols, CHANNELS[name])
    if name == "index":
        return torch.full(shape, _INDEX_POISON, dtype=torch.int64,
                          device="cuda")
    if name == "mask":
        return torch.full(shape, 0x77, dtype=torch.uint8, device="cuda")
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def poisoned(name, t):
    """Boolean tensor: which elements of map `name` still hold the poison."""
    if name == "index":
        return t == _INDEX_POISON
    if name == "mask":
        return t == 0x77
    return torch.isnan(t)


def assert_clean(out):
    for name, t in out.items():
        left = int(poisoned(name, t).sum())
        assert left == 0, "%s: %d elements never written" % (name, left)


def _finish(out, check):
    # (`mask` stays uint8: 0 / 1 once written)
    if check:
        assert_clean(out)
    return out


def ray_cast(g, keys, K, T, w, h, attrs, depth_scale, depth_min, depth_max,
             weight_threshold, trunc, down=8, check=True):
    """o3dmi_vbg_ray_cast: explicit keys {n,3} int32 on the device and a
    caller-owned range map (returned as "range")."""
    K, T = host_mat(K, (3, 3), "intrinsic"), host_mat(T, (4, 4), "extrinsic")
    assert keys.is_cuda and keys.dtype == torch.int32 and keys.is_contiguous()
    out = {a: alloc(a, h, w) for a in attrs}
    out["range"] = alloc("range", h // down, w // down)
    p = [_lib.ptr(out.get(a)) for a in _ORDER]
    _lib.check(_lib.lib().o3dmi_vbg_ray_cast(
        g._g, _lib.ptr(keys), keys.shape[0], _lib.f64p(K), _lib.f64p(T),
        int(w), int(h), _lib.ptr(out["range"]), *p, C.c_float(depth_scale),
        C.c_float(depth_min), C.c_float(depth_max),
        C.c_float(weight_threshold), C.c_float(trunc), int(down), stream()),
        "o3dmi_vbg_ray_cast")
    return _finish(out, check)


def ray_cast_last_frame(g, K, T, w, h, attrs, depth_scale, depth_min,
                        depth_max, weight_threshold, trunc, down=8,
                        check=True):
    """o3dmi_vbg_ray_cast_dev with NULL keys and a NULL range map: the grid's
    own last-frame block list and its own, self-cleaning, range map."""
    K, T = host_mat(K, (3, 3), "intrinsic"), host_mat(T, (4, 4), "extrinsic")
    out = {a: alloc(a, h, w) for a in attrs}
    p = [_lib.ptr(out.get(a)) for a in _ORDER]
    _lib.check(_lib.lib().o3dmi_vbg_ray_cast_dev(
        g._g, None, 0, None, _lib.f64p(K), _lib.f64p(T), int(w), int(h), None,
        *p, C.c_float(depth_scale), C.c_float(depth_min),
        C.c_float(depth_max), C.c_float(weight_threshold), C.c_float(trunc),
        int(down), stream()), "o3dmi_vbg_ray_cast_dev")
    return _finish(out, check)


def ray_cast_rows(g, range_map, K, T, w, h, row_begin, row_end, attrs,
                  depth_scale, depth_min, depth_max, weight_threshold, trunc,
                  down=8):
    """o3dmi_vbg_raycast_rows over the grid's own buffers: rows [row_begin,
    row_end) of whole-image maps; the rows outside keep the poison (nothing
    is checked here)."""
    K, T = host_mat(K, (3, 3), "intrinsic"), host_mat(T, (4, 4), "extrinsic")
    L = _lib.lib()
    tsdf, weight = g.attribute("tsdf"), g.attribute("weight")
    color = g.attribute("color") if "color" in attrs else None
    out = {a: alloc(a, h, w) for a in attrs}
    p = [_lib.ptr(out.get(a)) for a in _ORDER]
    _lib.check(L.o3dmi_vbg_raycast_rows(
        C.c_void_p(L.o3dmi_vbg_hashmap(g._g)), _lib.ptr(tsdf),
        _lib.ptr(weight), _lib.ptr(color),
        _lib.F32 if weight.dtype == torch.float32 else _lib.U16,
        _lib.ptr(range_map), *p, _lib.f64p(K), _lib.f64p(T), int(h), int(w),
        int(row_begin), int(row_end), g.block_resolution,
        C.c_float(g.voxel_size), C.c_float(depth_scale), C.c_float(depth_min),
        C.c_float(depth_max), C.c_float(weight_threshold), C.c_float(trunc),
        int(down), stream()), "o3dmi_vbg_raycast_rows")
    return out
