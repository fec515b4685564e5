"""CPU restatement (numpy) of ExtractTriangleMeshCPU, the reference's
marching cubes (cpp/open3d/t/geometry/kernel/VoxelBlockGridImpl.h:1383-1783,
helpers DeviceGetLinearIdx / DeviceGetNormal :94-149), emitting the GPU's
deterministic order: vertices by (active block in ascending buffer index,
voxel, axis), triangles by (active block, voxel, table order).

The table is an argument, (edge_owner {12,4}, tri_table {256,16},
tri_count {256}), so the same passes run with the project's generated table
(tools/gen_mc_tables.py). Pass 0 is restated in its scatter form (every valid
cube marks its crossing edges), independent of the GPU's gather form."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def project_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mc_tables as g
    finally:
        sys.path.pop(0)
    edge, tri, cnt = g.tables()
    return (np.array(g.EDGE_OWNER, np.int64), tri.astype(np.int64),
            cnt.astype(np.int64), np.array(g.CORNERS, np.int64), edge)


def extract_triangle_mesh(keys, active, tsdf, weight, color, res, voxel_size,
                          weight_threshold, table=None):
    """keys {cap,3} int32 (by buffer index), active = buffer indices,
    tsdf / weight {cap, R^3} (weight float32 or uint16), color {cap, R^3, 3}
    or None -> dict(positions, normals[, colors], indices, block_vertices,
    block_triangles, cube_triangles). cube_triangles: the triangle count of
    every cube that has triangles, in output order."""
    if table is None:
        table = project_table()
    edge_owner, tri_table, tri_count, corners, edge_table = table
    R = int(res)
    R3 = R ** 3
    f32 = np.float32
    active = np.sort(np.asarray(active, np.int64))
    n = active.shape[0]
    tsdf = np.asarray(tsdf, f32).reshape(-1)
    weight = np.asarray(weight).reshape(-1)
    if color is not None:
        color = np.asarray(color).reshape(-1, 3)
    empty = {"positions": np.zeros((0, 3), f32),
             "normals": np.zeros((0, 3), f32),
             "indices": np.zeros((0, 3), np.int32),
             "block_vertices": np.zeros(n, np.int64),
             "block_triangles": np.zeros(n, np.int64),
             "cube_triangles": np.zeros(0, np.int64)}
    if color is not None:
        empty["colors"] = np.zeros((0, 3), f32)
    if n == 0:
        return empty
    # BufferRadiusNeighbors (VoxelBlockGrid.cpp:22-51): nb[p, dx + 3dy + 9dz]
    lut = {tuple(int(v) for v in keys[b]): int(b) for b in active}
    nb = np.full((n, 27), -1, np.int64)
    for p, b in enumerate(active):
        k = keys[b]
        for t in range(27):
            d = (t % 3 - 1, (t // 3) % 3 - 1, t // 9 - 1)
            nb[p, t] = lut.get((int(k[0]) + d[0], int(k[1]) + d[1],
                                int(k[2]) + d[2]), -1)
    inv = {b: p for p, b in enumerate(active)}
    pos_of = np.vectorize(lambda b: inv.get(int(b), -1), otypes=[np.int64])

    vox = np.arange(R3, dtype=np.int64)
    xv = np.tile(vox % R, n)
    yv = np.tile((vox // R) % R, n)
    zv = np.tile(vox // (R * R), n)
    pw = np.repeat(np.arange(n, dtype=np.int64), R3)  # workload block

    def linear_idx(xo, yo, zo, p):
        """DeviceGetLinearIdx (:94-121); -1 = neighbour block absent."""
        xn, yn, zn = (xo + R) % R, (yo + R) % R, (zo + R) % R
        t = (np.sign(xo - xn) + 1) + (np.sign(yo - yn) + 1) * 3 + \
            (np.sign(zo - zn) + 1) * 9
        b = nb[p, t]
        li = ((b * R + zn) * R + yn) * R + xn
        return np.where(b < 0, -1, li)

    def get_normal(xo, yo, zo, p, nrm):
        """DeviceGetNormal (:123-149): a component is only overwritten when
        both neighbours exist."""
        for ax in range(3):
            d = [0, 0, 0]
            d[ax] = 1
            lp = linear_idx(xo + d[0], yo + d[1], zo + d[2], p)
            ln = linear_idx(xo - d[0], yo - d[1], zo - d[2], p)
            ok = (lp >= 0) & (ln >= 0)
            v = tsdf[np.where(ok, lp, 0)] - tsdf[np.where(ok, ln, 0)]
            nrm[ok, ax] = v[ok]

    # ---- pass 0 (:1459-1529): cube table index per voxel, edges marked
    table_idx = np.zeros(n * R3, np.int64)
    valid = np.ones(n * R3, bool)
    for i in range(8):
        li = linear_idx(xv + corners[i, 0], yv + corners[i, 1],
                        zv + corners[i, 2], pw)
        ok = li >= 0
        lic = np.where(ok, li, 0)
        w = weight[lic].astype(f32)
        valid &= ok & ~(w <= f32(weight_threshold))
        table_idx |= np.where(tsdf[lic] < 0, 1 << i, 0)
    table_idx = np.where(valid, table_idx, 0)
    marked = np.zeros(n * R3 * 3, bool)
    cubes = np.nonzero(valid & (table_idx != 0) & (table_idx != 255))[0]
    mask = edge_table[table_idx[cubes]]

    def owner(cube_ids, j):
        """(position, voxel) owning edge j of the cubes, and the edge axis."""
        xo = xv[cube_ids] + edge_owner[j, 0]
        yo = yv[cube_ids] + edge_owner[j, 1]
        zo = zv[cube_ids] + edge_owner[j, 2]
        dxb, dyb, dzb = xo // R, yo // R, zo // R
        t = (dxb + 1) + (dyb + 1) * 3 + (dzb + 1) * 9
        b = nb[pw[cube_ids], t]
        p = pos_of(b) if b.size else b
        v = ((zo - dzb * R) * R + (yo - dyb * R)) * R + (xo - dxb * R)
        return p * R3 + v, edge_owner[j, 3]

    for j in range(12):
        c = cubes[(mask >> j) & 1 == 1]
        if c.size == 0:
            continue
        w, ax = owner(c, j)
        marked[w * 3 + ax] = True
    # ---- pass 1: count; vertices numbered in (block, voxel, axis) order
    vid = np.full(n * R3 * 3, -1, np.int64)
    sel = np.nonzero(marked)[0]
    nv = sel.shape[0]
    vid[sel] = np.arange(nv)
    if nv > 0x7FFFFFFF:
        raise OverflowError("more than INT32_MAX vertices")
    # ---- pass 2 (:1567-1678)
    wv = sel // 3
    positions = np.zeros((nv, 3), f32)
    normals = np.zeros((nv, 3), f32)
    colors = np.zeros((nv, 3), f32) if color is not None else None
    has = marked.reshape(-1, 3)
    vox_any = np.nonzero(has.any(axis=1))[0]
    no = np.zeros((vox_any.shape[0], 3), f32)
    get_normal(xv[vox_any], yv[vox_any], zv[vox_any], pw[vox_any], no)
    ne = np.zeros((vox_any.shape[0], 3), f32)  # carried over the axes
    blk = active[pw[vox_any]]
    lin_o = blk * R3 + vox_any % R3
    tsdf_o = tsdf[lin_o]
    one = f32(1)
    for e in range(3):
        m = has[vox_any, e]
        if not m.any():
            continue
        xe = xv[vox_any][m] + (e == 0)
        ye = yv[vox_any][m] + (e == 1)
        ze = zv[vox_any][m] + (e == 2)
        lin_e = linear_idx(xe, ye, ze, pw[vox_any][m])
        assert (lin_e >= 0).all()
        to = tsdf_o[m]
        ratio = (f32(0) - to) / (tsdf[lin_e] - to)
        idx = vid[vox_any[m] * 3 + e]
        xyz = keys[blk[m]].astype(np.int64) * R + np.stack(
            [xv[vox_any][m], yv[vox_any][m], zv[vox_any][m]], 1)
        for k in range(3):
            positions[idx, k] = f32(voxel_size) * (
                xyz[:, k].astype(f32) + ratio * f32(int(e == k)))
        ne_m = ne[m]
        get_normal(xe, ye, ze, pw[vox_any][m], ne_m)
        ne[m] = ne_m
        no_m = no[m]
        nx = (one - ratio) * no_m[:, 0] + ratio * ne_m[:, 0]
        ny = (one - ratio) * no_m[:, 1] + ratio * ne_m[:, 1]
        nz = (one - ratio) * no_m[:, 2] + ratio * ne_m[:, 2]
        norm = (np.sqrt(nx * nx + ny * ny + nz * nz).astype(np.float64) +
                1e-5).astype(f32)
        normals[idx, 0] = nx / norm
        normals[idx, 1] = ny / norm
        normals[idx, 2] = nz / norm
        if colors is not None:
            co = color[lin_o[m]].astype(f32)
            ce = color[lin_e].astype(f32)
            for k in range(3):
                colors[idx, k] = ((one - ratio) * co[:, k] +
                                  ratio * ce[:, k]) / f32(255.0)
    # ---- pass 3 (:1680-1776): triangles of the valid cubes in table order
    ntri = np.where(valid, tri_count[table_idx], 0)
    cube_ids = np.repeat(np.arange(n * R3), ntri)
    starts = np.cumsum(ntri) - ntri
    t = np.arange(cube_ids.shape[0]) - np.repeat(starts, ntri)
    tris = np.zeros((cube_ids.shape[0], 3), np.int64)
    cases = table_idx[cube_ids]
    for k in range(3):
        edges = tri_table[cases, 3 * t + k]
        for j in range(12):
            m = edges == j
            if not m.any():
                continue
            w, ax = owner(cube_ids[m], j)
            tris[m, k] = vid[w * 3 + ax]
    assert (tris >= 0).all()
    out = {"positions": positions, "normals": normals,
           "indices": tris.astype(np.int32),
           "block_vertices": has.reshape(n, -1).sum(1).astype(np.int64),
           "block_triangles": ntri.reshape(n, R3).sum(1).astype(np.int64),
           "cube_triangles": ntri[ntri > 0].astype(np.int64)}
    if colors is not None:
        out["colors"] = colors
    return out
