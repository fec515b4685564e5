"""numpy Float32 restatement of slac::ControlGrid (t/pipelines/slac/
ControlGrid.cpp) and of the point-cloud projection (t/geometry/kernel/
PointCloudCUDA.cu:26-160), in the operation order the kernels state.

Nodes are identified by their keys: a grid is a dict key -> current position,
never a buffer index. Every array is float32; sums are written out term by
term so that numpy cannot reorder them.
"""
import numpy as np

F = np.float32
KEY_LIMIT = 1 << 20  # the hash's key range

# corner nb = x_sel << 2 | y_sel << 1 | z_sel
CORNERS = np.array([[(nb >> 2) & 1, (nb >> 1) & 1, nb & 1] for nb in range(8)],
                   np.int32)
# -x +x -y +y -z +z
DIRECTIONS = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0],
                       [0, 0, -1], [0, 0, 1]], np.int32)


def quantize(points, grid_size):
    """(floor(p / grid_size) as float32, the residual, valid): valid is False
    for non-finite rows and for cells outside the key range."""
    p = np.asarray(points, F)
    with np.errstate(all="ignore"):
        q = p / F(grid_size)
        fl = np.floor(q)
        res = q - fl
        ok = np.isfinite(fl) & (fl >= F(-KEY_LIMIT)) & (fl <= F(KEY_LIMIT - 2))
    return fl, res, ok.all(1)


def touch(points, grid_size):
    """The node keys a Touch of `points` creates ({m,3} int32, sorted rows)
    and their values (vals + dt) * grid_size."""
    fl, _, ok = quantize(points, grid_size)
    fl = fl[ok]
    keys = (fl.astype(np.int32)[:, None, :] + CORNERS[None]).reshape(-1, 3)
    vals = ((fl[:, None, :] + CORNERS[None].astype(F)) *
            F(grid_size)).reshape(-1, 3).astype(F)
    keys, first = np.unique(keys, axis=0, return_index=True)
    return keys, vals[first]


def key_set(keys):
    return {tuple(int(v) for v in k) for k in np.asarray(keys)}


def anchor_key(keys):
    """Compactify's anchor: position size / 2 of the keys sorted by (z, y, x)."""
    keys = np.asarray(keys)
    order = np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))
    return tuple(int(v) for v in keys[order[len(order) // 2]])


def neighbor_masks(keys):
    """{n,6} bool: key + DIRECTIONS[d] is a node."""
    present = key_set(keys)
    return np.array([[tuple(int(v) for v in (k + d)) in present
                      for d in DIRECTIONS] for k in np.asarray(keys)], bool)


def parameterize(points, grid_size, nodes, normals=None):
    """nodes: a set (or dict) of keys. Returns dict(valid {n} bool, keys
    {m,8,3} int32 of the survivors' corners, vertex {m,8}, normal {m,8} or
    None), survivors in input order."""
    fl, res, ok = quantize(points, grid_size)
    base = np.where(ok[:, None], fl, 0).astype(np.int32)
    corner_keys = base[:, None, :] + CORNERS[None]
    valid = ok.copy()
    for i in np.nonzero(ok)[0]:
        valid[i] = all(tuple(int(v) for v in k) in nodes
                       for k in corner_keys[i])
    r = np.stack([F(1) - res, res], -1).astype(F)[valid]  # {m,3,2}
    m = r.shape[0]
    vertex = np.empty((m, 8), F)
    normal = None if normals is None else np.empty((m, 8), F)
    nm = None if normals is None else np.asarray(normals, F)[valid]
    for nb, (xs, ys, zs) in enumerate(CORNERS):
        rx, ry, rz = r[:, 0, xs], r[:, 1, ys], r[:, 2, zs]
        vertex[:, nb] = (rx * ry) * rz
        if nm is not None:
            sx, sy, sz = F(xs * 2.0 - 1.0), F(ys * 2.0 - 1.0), F(zs * 2.0 - 1.0)
            a = ((sx * nm[:, 0]) * ry) * rz
            b = ((sy * nm[:, 1]) * rx) * rz
            c = ((sz * nm[:, 2]) * rx) * ry
            normal[:, nb] = (a + b) + c
    return dict(valid=valid, keys=corner_keys[valid], vertex=vertex,
                normal=normal)


def corner_positions(corner_keys, grid):
    """{m,8,3} current positions of the corner keys from the dict `grid`."""
    flat = np.asarray(corner_keys).reshape(-1, 3)
    return np.array([grid[tuple(int(v) for v in k)] for k in flat],
                    F).reshape(-1, 8, 3)


def interpolate(corners, ratios):
    """sum_k ratio_k * corner_k in k order."""
    acc = ratios[:, 0, None] * corners[:, 0]
    for k in range(1, 8):
        acc = acc + ratios[:, k, None] * corners[:, k]
    return acc.astype(F)


def deform(corners, vertex, normal=None):
    pos = interpolate(corners, vertex)
    if normal is None:
        return pos, None
    v = interpolate(corners, normal)
    with np.errstate(all="ignore"):
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) +
                         v[:, 2] * v[:, 2])
        return pos, (v / length[:, None]).astype(F)


def identity_grid(keys, grid_size):
    return {tuple(int(v) for v in k): (np.asarray(k).astype(F) * F(grid_size))
            for k in np.asarray(keys)}


# ---- camera (t/geometry/kernel/GeometryIndexer.h, float32) -----------------

def inverse_transformation(T):
    """t/geometry/Utility.h:77-120, float64."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3].T
    out = np.eye(4)
    out[:3, :3] = R
    for r in range(3):
        out[r, 3] = -(R[r, 0] * T[0, 3] + R[r, 1] * T[1, 3] +
                      R[r, 2] * T[2, 3])
    return out


def _rigid(T, x, y, z):
    e = np.asarray(T, np.float64).astype(F)
    return tuple(x * e[r, 0] + y * e[r, 1] + z * e[r, 2] + e[r, 3]
                 for r in range(3))


def _round_half_away(x):
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= F(0.5), np.sign(x), 0)).astype(F)


def color_to_float(color):
    """Image::To(Float32) of a UInt8 image: scale 1/255, clamped from below
    to the smallest normal float."""
    c = np.asarray(color)
    if c.dtype == np.float32:
        return c
    return np.maximum(c.astype(F) * F(1.0 / 255) + F(0), F(1.17549435e-38))


def unproject(depth, K, T, depth_scale, depth_max):
    """World points of the valid pixels in row-major order, and the linear
    indices of those pixels."""
    depth = np.asarray(depth)
    rows, cols = depth.shape
    d = depth.astype(F).reshape(-1) / F(depth_scale)
    with np.errstate(invalid="ignore"):
        valid = (d > 0) & (d < F(depth_max))
    pix = np.nonzero(valid)[0]
    d = d[pix]
    u, v = (pix % cols).astype(F), (pix // cols).astype(F)
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    xc = (u - cx) * d / fx
    yc = (v - cy) * d / fy
    x, y, z = _rigid(inverse_transformation(T), xc, yc, d)
    return np.stack([x, y, z], 1).astype(F), pix


def project(points, K, T, rows, cols, depth_scale, depth_max, colors=None,
            return_hits=False):
    """Per pixel the minimum over (d, point index); empty pixels are 0."""
    p = np.asarray(points, F).reshape(-1, 3)
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    with np.errstate(all="ignore"):
        xc, yc, zc = _rigid(T, p[:, 0], p[:, 1], p[:, 2])
        inv_z = F(1) / zc
        u = _round_half_away(fx * xc * inv_z + cx)
        v = _round_half_away(fy * yc * inv_z + cy)
        keep = ((v >= 0) & (u >= 0) & (v <= F(rows - 1)) & (u <= F(cols - 1))
                & ~(zc <= 0) & ~(zc > F(depth_max)))
    idx = np.nonzero(keep)[0]
    pixel = v[idx].astype(np.int64) * cols + u[idx].astype(np.int64)
    d = (zc[idx] * F(depth_scale)).astype(F)
    order = np.lexsort((idx, d, pixel))
    pixel_s = pixel[order]
    first = np.ones(len(order), bool)
    first[1:] = pixel_s[1:] != pixel_s[:-1]
    win = order[first]
    depth = np.zeros(rows * cols, F)
    depth[pixel[win]] = d[win]
    out = [depth.reshape(rows, cols)]
    if colors is not None:
        color = np.zeros((rows * cols, 3), F)
        color[pixel[win]] = np.asarray(colors, F)[idx[win]]
        out.append(color.reshape(rows, cols, 3))
    if return_hits:
        out.append(np.bincount(pixel, minlength=rows * cols))
    return out[0] if len(out) == 1 else tuple(out)


def deform_image(depth, color, K, T, depth_scale, depth_max, grid_size, grid):
    """ControlGrid::Deform of a depth (color None) or RGB-D image through the
    dict `grid`: the unfused chain."""
    rows, cols = np.asarray(depth).shape
    pts, pix = unproject(depth, K, T, depth_scale, depth_max)
    par = parameterize(pts, grid_size, grid)
    pos, _ = deform(corner_positions(par["keys"], grid), par["vertex"])
    cl = None
    if color is not None:
        cl = color_to_float(color).reshape(-1, 3)[pix][par["valid"]]
    return project(pos, K, T, rows, cols, depth_scale, depth_max, cl)
