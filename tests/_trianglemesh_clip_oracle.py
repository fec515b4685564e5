"""A literal numpy / Python restatement of the ClipPlane / SlicePlane rules of
include/o3d_mi355x_host.h, in float64 with the stated operation order; the
narrowing to the position dtype happens once, on the way out.

  signed value   s_i = ((n.x (x_i - o.x) + n.y (y_i - o.y)) + n.z (z_i - o.z))
  inside         s_i >= c (clip: c = 0)
  rotation       one inside: the inside vertex first; two inside: the outside
                 vertex last; (a, b, c) with the edges ab, bc, ca, whose slots
                 are 3 t + (r + 0, 1, 2) % 3 for the rotation r
  cut point      of a crossing edge with the inside end u: vertex u itself if
                 s_u == c, else the point of the unordered edge (lo, hi):
                 t = (c - s_lo) / (s_hi - s_lo), x_lo + t * (x_hi - x_lo)
  a point's key  (u, u) or (lo, hi); a piece or line that names a key twice is
                 dropped and numbers nothing

Clip numbers the old vertices the kept pieces name first (ascending), then
the edge points by the lowest slot among the kept pieces' uses. Slice numbers
every point of a contour that way, contour after contour.
"""
import numpy as np


def signed_values(positions, point, normal):
    p = np.asarray(positions).astype(np.float64)
    o = [float(x) for x in point]
    n = [float(x) for x in normal]
    with np.errstate(all="ignore"):
        return ((n[0] * (p[:, 0] - o[0]) + n[1] * (p[:, 1] - o[1])) +
                n[2] * (p[:, 2] - o[2]))


def _key(x, y, s, c):
    """The point of the crossing edge with the ends x, y."""
    u = x if s[x] >= c else y
    if s[u] == c:
        return (u, u)
    return (min(x, y), max(x, y))


def _rotate(t, row, s, c):
    """-> nin, (a, b, c), the slots of (ab, bc, ca)."""
    ins = [bool(s[i] >= c) for i in row]
    nin = sum(ins)
    if nin == 1:
        r = ins.index(True)
    elif nin == 2:
        r = (ins.index(False) + 1) % 3
    else:
        r = 0
    v = [int(row[(r + k) % 3]) for k in range(3)]
    return nin, v, [3 * t + (r + k) % 3 for k in range(3)]


def cut_parameter(c, s_lo, s_hi):
    with np.errstate(all="ignore"):
        return (np.float64(c) - s_lo) / (s_hi - s_lo)


def mix(x_lo, x_hi, t):
    """The attribute statement, per component in float64."""
    with np.errstate(all="ignore"):
        return x_lo + t * (x_hi - x_lo)


def _point_rows(keys, s, c, attrs):
    """-> source {n,2} int64, t {n} float64, the attribute rows (float64) of
    the points `keys`."""
    n = len(keys)
    source = np.asarray(keys, np.int64).reshape(n, 2)
    t = np.zeros(n, np.float64)
    rows = [np.zeros((n, 3), np.float64) for _ in attrs]
    for i, (lo, hi) in enumerate(keys):
        if lo != hi:
            t[i] = cut_parameter(c, s[lo], s[hi])
        for a, out in zip(attrs, rows):
            out[i] = a[lo] if lo == hi else mix(a[lo], a[hi], t[i])
    return source, t, rows


def _number(uses):
    """uses: (key, slot) pairs -> the keys in ascending lowest slot."""
    lowest = {}
    for key, slot in uses:
        if key not in lowest or slot < lowest[key]:
            lowest[key] = slot
    return sorted(lowest, key=lowest.get)


def _wide(arrays):
    return [np.asarray(a).astype(np.float64) for a in arrays]


def clip_plane(positions, triangles, point, normal, normals=None,
               colors=None):
    """-> dict(positions, normals, colors (None when not given), triangles
    int64 {T,3}, triangle_source int64 {T}, vertex_source int64 {V,2},
    vertex_t float64 {V})."""
    positions = np.asarray(positions)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    s = signed_values(positions, point, normal)
    c = 0.0
    pieces = []  # (input triangle, [(key, slot or None)] * 3)
    for t, row in enumerate(tri):
        nin, (a, b, cc), (ab, bc, ca) = _rotate(t, row, s, c)
        va, vb, vc = ((a, a), None), ((b, b), None), ((cc, cc), None)
        if nin == 3:
            cand = [[va, vb, vc]]
        elif nin == 1:
            cand = [[va, (_key(a, b, s, c), ab), (_key(cc, a, s, c), ca)]]
        elif nin == 2:
            kbc = (_key(b, cc, s, c), bc)
            cand = [[va, vb, kbc], [va, kbc, (_key(cc, a, s, c), ca)]]
        else:
            cand = []
        for piece in cand:
            if len({k for k, _ in piece}) == 3:
                pieces.append((t, piece))
    refs = [ref for _, piece in pieces for ref in piece]
    old = sorted({k[0] for k, _ in refs if k[0] == k[1]})
    new = _number([(k, slot) for k, slot in refs if k[0] != k[1]])
    ident = {(u, u): i for i, u in enumerate(old)}
    ident.update({k: len(old) + i for i, k in enumerate(new)})
    keys = [(u, u) for u in old] + new
    given = [a for a in (positions, normals, colors) if a is not None]
    source, tt, rows = _point_rows(keys, s, c, _wide(given))
    rows = [r.astype(positions.dtype) for r in rows]
    rows = iter(rows)
    out = {name: (next(rows) if a is not None else None)
           for name, a in (("positions", positions), ("normals", normals),
                           ("colors", colors))}
    out["triangles"] = np.asarray(
        [[ident[k] for k, _ in piece] for _, piece in pieces],
        np.int64).reshape(-1, 3)
    out["triangle_source"] = np.asarray([t for t, _ in pieces], np.int64)
    out["vertex_source"] = source
    out["vertex_t"] = tt
    return out


def slice_plane(positions, triangles, point, normal, contour_values=(0.0,),
                normals=None, colors=None):
    """-> dict(positions, normals, colors (None when not given), lines int64
    {L,2}, line_triangle int64 {L}, line_contour int32 {L}, point_source int64
    {P,2}, point_t float64 {P})."""
    positions = np.asarray(positions)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    s = signed_values(positions, point, normal)
    given = [a for a in (positions, normals, colors) if a is not None]
    wide = _wide(given)
    lines, line_tri, line_contour = [], [], []
    sources, ts = [], []
    rows_all = [[] for _ in given]
    base = 0
    for ci, c in enumerate(contour_values):
        c = float(c)
        kept = []
        for t, row in enumerate(tri):
            nin, (a, b, cc), (ab, bc, ca) = _rotate(t, row, s, c)
            if nin == 1:
                ends = [(_key(a, b, s, c), ab), (_key(cc, a, s, c), ca)]
            elif nin == 2:
                ends = [(_key(b, cc, s, c), bc), (_key(cc, a, s, c), ca)]
            else:
                continue
            if ends[0][0] != ends[1][0]:
                kept.append((t, ends))
        keys = _number([end for _, ends in kept for end in ends])
        ident = {k: base + i for i, k in enumerate(keys)}
        for t, ends in kept:
            lines.append([ident[ends[0][0]], ident[ends[1][0]]])
            line_tri.append(t)
            line_contour.append(ci)
        source, tt, rows = _point_rows(keys, s, c, wide)
        sources.append(source)
        ts.append(tt)
        for acc, r in zip(rows_all, rows):
            acc.append(r)
        base += len(keys)
    rows = iter([np.concatenate(acc + [np.zeros((0, 3))]).astype(
        positions.dtype) for acc in rows_all])
    out = {name: (next(rows) if a is not None else None)
           for name, a in (("positions", positions), ("normals", normals),
                           ("colors", colors))}
    out["lines"] = np.asarray(lines, np.int64).reshape(-1, 2)
    out["line_triangle"] = np.asarray(line_tri, np.int64)
    out["line_contour"] = np.asarray(line_contour, np.int32)
    out["point_source"] = np.concatenate(
        sources + [np.zeros((0, 2), np.int64)])
    out["point_t"] = np.concatenate(ts + [np.zeros(0)])
    return out


def interpolate(attribute, source, t):
    """Any other floating vertex attribute {V, ...} carried by source / t: the
    statement of the cut point in float64, narrowed; an old vertex's row is a
    copy."""
    a = np.asarray(attribute)
    w = a.astype(np.float64)
    tt = t.reshape((-1,) + (1,) * (a.ndim - 1))
    lo, hi = source[:, 0], source[:, 1]
    out = mix(w[lo], w[hi], tt)
    same = lo == hi
    out[same] = w[lo[same]]
    return out.astype(a.dtype)
