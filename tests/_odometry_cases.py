"""Input builders for the RGB-D odometry tests (test_odometry_oracle.py pins
them to the reference bodies on the CPU, test_odometry_gpu.py runs the same
sets through the HIP kernels).

Crafted one-level sets. A few rows by a few tens of columns, K with
power-of-two focal lengths, planar source depth, T = identity + a translation,
target = source + per-column offsets. Unless a builder says otherwise every
value is a dyadic rational with few bits, so the float32 per-pixel arithmetic
is exact and the residual of a pixel is the offset written for it. Each builder
has one regime switch; `off` states of the switch give the input the regime
test compares against.

A case is a dict: L (K, T and the eleven maps, the keyword names of
orc.odometry_sums), kw (trunc and the two Huber deltas), info_thr (square
distance threshold of the information matrix), exact (True when every term
of the point-to-plane sums and of the information matrix is a multiple of
2^-40 below 2^12: float64 sums of such terms are exact in any order).
"""
import functools

import numpy as np

import _oracle as orc

NAN = float("nan")
ROWS, COLS = 6, 40
K0 = np.array([[64.0, 0, 20.0], [0, 64.0, 3.0], [0, 0, 1.0]])
EPS = 2.0 ** -10

# not unit length on purpose: the kernels never normalise, dyadic components
# keep r and J exact, and nz = -1 makes a pure z offset the residual itself
_NORMALS = np.array([[0, 0, -1], [0.5, 0, -1], [0, 0.5, -1],
                     [-0.5, 0.25, -1], [0.25, -0.5, -1]], np.float32)


def _grid(rows, cols):
    v, u = np.mgrid[0:rows, 0:cols]
    return u.astype(np.float64), v.astype(np.float64)


def _vertex(pu, pv, d, K):
    """Point at depth d on the ray through image position (pu, pv)."""
    d = np.broadcast_to(np.asarray(d, np.float64), np.shape(pu))
    x = (pu - K[0, 2]) * d / K[0, 0]
    y = (pv - K[1, 2]) * d / K[1, 1]
    return np.stack([x, y, d], -1).astype(np.float32)


def _translation(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


def _per_column(pattern, cols):
    return np.array([pattern[c % len(pattern)] for c in range(cols)])


def _assemble(K, T, source_vertex, target_depth, r_intensity,
              base_depth=2.0):
    """Target maps as functions of the target pixel. The target vertex is the
    point of the plane z = base_depth on the pixel's ray, moved along z to
    target_depth: a source point that lands on the pixel centre differs from
    it in z alone, and every normal has nz = -1, so the point-to-plane
    residual is target_depth - Tz whatever nx and ny are. r_intensity
    {rows, cols} is target - source intensity at the same pixel
    (T_I = max(r, 0), S_I = max(-r, 0))."""
    rows, cols = target_depth.shape
    u, v = _grid(rows, cols)
    ui, vi = u.astype(int), v.astype(int)
    f = np.float32
    r_intensity = np.broadcast_to(r_intensity, (rows, cols))
    return dict(
        K=K, T=T, source_vertex=source_vertex.astype(f),
        target_vertex=np.concatenate(
            [_vertex(u, v, base_depth, K)[..., :2],
             target_depth[..., None].astype(f)], -1),
        target_normal=_NORMALS[(ui + 3 * vi) % 5].copy(),
        source_depth=np.ascontiguousarray(source_vertex[..., 2]).astype(f),
        target_depth=target_depth.astype(f),
        source_intensity=np.maximum(-r_intensity, 0).astype(f),
        target_intensity=np.maximum(r_intensity, 0).astype(f),
        target_depth_dx=(0.125 * ((ui + 2 * vi) % 5 - 2)).astype(f),
        target_depth_dy=(0.125 * ((2 * ui + vi) % 3 - 1)).astype(f),
        target_intensity_dx=(0.25 * ((3 * ui + vi) % 5 - 2)).astype(f),
        target_intensity_dy=(0.25 * ((ui + 2 * vi) % 7 - 3)).astype(f))


def _case(L, trunc, depth_delta, intensity_delta, info_thr, exact=True, **kw):
    return dict(L=L, kw=dict(depth_outlier_trunc=trunc,
                             depth_huber_delta=depth_delta,
                             intensity_huber_delta=intensity_delta),
                info_thr=info_thr, exact=exact, **kw)


# ---------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------
def huber_zones(delta=0.75, scale=1.0, mid=0.875, tail=1.5, imid=0.75,
                itail=1.5, drop=()):
    """Residuals in the three zones of HuberDeriv, both signs: |r| < delta,
    delta <= |r| < 1 (the reference's Sign(int(r)) is 0 there: derivative 0)
    and 1 <= |r| <= trunc = 3 (derivative +-delta). Depth and intensity
    residuals of a column lie in the same zone (intensity delta 0.5), columns
    repeat with period 14: 4 small, 2 mid (+-mid / +-imid), 8 tail (among
    them +-tail / +-itail). `drop` names zones whose source vertices are
    made NaN. scale = 1: values exact, with +-1.0 and +-1.25 (== delta 1.25)
    in the tail. scale = 1 / 0.707 is for the hybrid method, which multiplies
    its residuals by 0.707f: the written values are then met to a few ulp
    only, so none of them sits on a zone border."""
    exact = scale == 1.0
    one = 1.0 if exact else 1.125
    zones = {"small": ((0.5, -0.5, 0.25, 0.0), (0.25, -0.25, 0.0, 0.125)),
             "mid": ((mid, -mid), (imid, -imid)),
             "tail": ((one, -one, tail, -tail, 2.0, -2.0) +
                      ((1.25, -1.25) if exact else (1.375, -1.375)),
                      (one, -one, itail, -itail, one, -one, 1.25, -1.25))}
    order = ("small", "mid", "tail")
    off = _per_column([x * scale for z in order for x in zones[z][0]], COLS)
    ri = _per_column([x * scale for z in order for x in zones[z][1]], COLS)
    zone_of = _per_column([z for z in order for _ in zones[z][0]], COLS)
    u, v = _grid(ROWS, COLS)
    sv = _vertex(u, v, 2.0, K0)
    sv[:, np.isin(zone_of, drop)] = NAN
    L = _assemble(K0, np.eye(4), sv, 2.0 + np.tile(off, (ROWS, 1)),
                  np.tile(ri, (ROWS, 1)))
    return _case(L, 3.0, delta, 0.5, 16.0, exact=exact,
                 n_zone={z: int((zone_of == z).sum()) * ROWS for z in order})


def _x707(target):
    """float32 x with float32(0.707f * x) == target exactly (the hybrid
    method scales its residuals by 0.707f before the Huber test)."""
    x = np.float32(target) / np.float32(0.707)
    for _ in range(64):
        p = np.float32(np.float32(0.707) * x)
        if p == np.float32(target):
            return float(x)
        x = np.nextafter(x, np.float32(np.inf if p < target else -np.inf))
    raise AssertionError("no float32 x with 0.707f * x == %r" % target)


# columns (mod 10) of `thresholds` whose Huber derivative is 0 because |r| ==
# delta, per method; hybrid: r_I == delta through the 0.707f scale, r_D == 0
THRESHOLD_DELTA_COLUMNS = {0: (4, 5), 1: (4, 5), 2: (6, 7)}


def thresholds(at_trunc=True, at_delta=True, drop_columns=()):
    """|r| exactly equal to trunc = 0.5 (kept: the test is >) and exactly equal
    to delta = 0.25 (Huber tail: the test is <, and Sign(int(0.25)) = 0 makes
    the derivative 0). Off: the same columns moved 2^-10 to the other side.
    The intensity residuals hit 0.25 for method 1 and 0.707f * x == 0.25 for
    the hybrid method. Source vertices of the columns `drop_columns` (mod 10)
    are made NaN."""
    t = 0.5 if at_trunc else 0.5 + EPS
    d = 0.25 if at_delta else 0.25 - EPS
    x = _x707(0.25) if at_delta else _x707(0.25) * (1 - EPS)
    off = _per_column((0.125, -0.125, t, -t, d, -d, 0.0, 0.0, 0.75, 0.375),
                      COLS)
    ri = _per_column((0.125, -0.125, 0.0, 0.125, d, -d, x, -x, 0.5, 0.0),
                     COLS)
    u, v = _grid(ROWS, COLS)
    sv = _vertex(u, v, 2.0, K0)
    sv[:, np.isin(np.arange(COLS) % 10, drop_columns)] = NAN
    L = _assemble(K0, np.eye(4), sv, 2.0 + np.tile(off, (ROWS, 1)),
                  np.tile(ri, (ROWS, 1)))
    return _case(L, 0.5, 0.25, 0.25, 0.25)


def behind_camera(neg=True, zero=True):
    """T = translation (0, 0, -1). Source depth 2 -> Tz = 1; columns with
    depth 0.5 -> Tz = -0.5 (they project to (40 - u, 6 - v): inside the image,
    residual <= trunc, so only the Tz < 0 test rejects them); columns with
    depth 1 -> Tz == 0 (Project yields +-inf, and NaN where Tx or Ty is 0,
    which includes the pixel on the principal point). Off: depth 2 there.
    The one Tz = 1 pixel that lands on (column cols, last row) is left
    invalid, so that even a column test that is off by one reads inside the
    maps."""
    d = _per_column((2.0, 2.0, 1.0 if zero else 2.0, 2.0,
                     0.5 if neg else 2.0, 2.0), COLS)
    off = _per_column((0.0, 0.25, -0.25, 0.125), COLS)
    u, v = _grid(ROWS, COLS)
    sv = _vertex(u, v, np.tile(d, (ROWS, 1)), K0)
    sv[4, 30] = NAN             # (2 u - 20, 2 v - 3) == (COLS, ROWS - 1)
    L = _assemble(K0, _translation(tz=-1.0), sv,
                  1.0 + np.tile(off, (ROWS, 1)), 0.25 * ((u + v) % 3 - 1),
                  base_depth=1.0)
    return _case(L, 2.0, 0.75, 0.5, 4.0)


def boundary(mode="on"):
    """T = lateral shift; crafted source vertices whose projections land at
    columns -0.5 (roundf -> -1: out), just above -0.5, cols - 1 + 0.49, just
    below cols - 0.5 (in) and cols - 0.5 (roundf -> cols: out), and the same
    for rows. mode "all_in" moves the outside landings to the nearest pixel
    centre inside, "all_out" moves the inside edge landings onto the outside
    position. Landings at column `cols` stay above the last row, so that even
    a column test that is off by one reads inside the maps. Returns n_out /
    n_in, the number of pixels of either kind."""
    assert mode in ("on", "all_in", "all_out")
    rows, cols = ROWS, COLS
    tx, ty = -1.0 / 64, 1.0 / 32

    def edges(n):
        lo, hi = -0.5, n - 0.5
        return [(lo, lo, 0.0), (lo + EPS, lo, None), (-0.49, lo, None),
                (n - 1 + 0.49, hi, None), (hi - EPS, hi, None),
                (hi, hi, n - 1.0)]

    def pick(pos, out_pos, in_pos):
        if in_pos is not None:       # an outside landing
            return in_pos if mode == "all_in" else pos
        return out_pos if mode == "all_out" else pos
    pu, pv = _grid(rows, cols)
    n_out = n_in = 0
    for row in (1, 2):
        for i, e in enumerate(edges(cols)):
            pu[row, 5 + i] = pick(*e)
            n_out += e[2] is not None
            n_in += e[2] is None
    for i, e in enumerate(edges(rows)):
        pv[4, 20 + i] = pick(*e)
        n_out += e[2] is not None
        n_in += e[2] is None
    pu[3, 30], pv[3, 30] = pick(-0.5 + EPS, -0.5, None), \
        pick(-0.5 + EPS, -0.5, None)                 # corner, inside
    n_in += 1
    sv = _vertex(pu, pv, 2.0, K0).astype(np.float64)
    sv[..., 0] -= tx
    sv[..., 1] -= ty
    off = _per_column((0.0, 0.25, -0.25, 0.125), cols)
    u, v = _grid(rows, cols)
    L = _assemble(K0, _translation(tx, ty), sv,
                  2.0 + np.tile(off, (rows, 1)), 0.25 * ((u + v) % 3 - 1))
    # -0.49 and cols - 1 + 0.49 are not dyadic: the sums are not exact
    return _case(L, 0.5, 0.125, 0.125, 0.5, exact=False, n_out=n_out,
                 n_in=n_in)


NAN_MAPS = ("target_vertex", "target_normal", "target_depth",
            "target_depth_dx", "target_depth_dy", "source_vertex")
# which results a NaN in that map alone may change: methods 0 / 1 / 2, "info"
NAN_AFFECTS = {"target_vertex": (0, "info"), "target_normal": (0,),
               "target_depth": (1, 2), "target_depth_dx": (2,),
               "target_depth_dy": (2,), "source_vertex": (0, 1, 2, "info")}
NAN_PIXELS = ((0, 0), (2, 7), (3, 19), (4, 20), (5, 39))


def nan_planted(which=None):
    """NaN at NAN_PIXELS of exactly one map (None: no NaN anywhere)."""
    assert which is None or which in NAN_MAPS
    off = _per_column((0.0, 0.25, -0.25, 0.125, -0.375), COLS)
    u, v = _grid(ROWS, COLS)
    L = _assemble(K0, np.eye(4), _vertex(u, v, 2.0, K0),
                  2.0 + np.tile(off, (ROWS, 1)), 0.25 * ((u + v) % 3 - 1))
    if which is not None:
        for r, c in NAN_PIXELS:
            L[which][r, c] = NAN
    return _case(L, 0.5, 0.125, 0.125, 0.5)


def rotated(on=True):
    """60 x 80, smooth surfaces with holes, maps made by the oracle's image
    ops. On: fx != fy, principal point off-centre, T with a rotation of a few
    degrees about each axis. Off: square K, identity T."""
    rows, cols = 60, 80
    if on:
        K = np.array([[70.0, 0, 41.3], [0, 65.5, 27.6], [0, 0, 1.0]])
        ax, ay, az = np.deg2rad([3.0, -2.0, 4.0])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)],
                       [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0],
                       [-np.sin(ay), 0, np.cos(ay)]])
        Rz = np.array([[np.cos(az), -np.sin(az), 0],
                       [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        T = np.eye(4)
        T[:3, :3] = Rz @ Ry @ Rx
        T[:3, 3] = (0.02, -0.01, 0.015)
    else:
        K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1.0]])
        T = np.eye(4)
    u, v = _grid(rows, cols)
    f = np.float32
    sd = (1.5 + 0.2 * np.sin(u / 9) + 0.15 * np.cos(v / 7)).astype(f)
    td = (sd + 0.01 * np.sin(u / 3 + v / 5)).astype(f)
    rng = np.random.default_rng(5)
    sd[rng.random(sd.shape) < 0.03] = NAN
    td[rng.random(td.shape) < 0.03] = NAN
    td[20:24, 50:60] = NAN
    si = (0.5 + 0.4 * np.sin(u / 5) * np.cos(v / 4)).astype(f)
    ti = (0.5 + 0.4 * np.sin((u + 1.5) / 5) * np.cos(v / 4)).astype(f)
    tdx, tdy = orc.filter_sobel(td)
    tix, tiy = orc.filter_sobel(ti)
    tv = orc.create_vertex_map(td, K, NAN)
    L = dict(K=K, T=T, source_vertex=orc.create_vertex_map(sd, K, NAN),
             target_vertex=tv, target_normal=orc.create_normal_map(tv, NAN),
             source_depth=sd, target_depth=td, source_intensity=si,
             target_intensity=ti, target_depth_dx=tdx, target_depth_dy=tdy,
             target_intensity_dx=tix, target_intensity_dy=tiy)
    return _case(L, 0.3, 0.05, 0.1, 0.09, exact=False)


CRAFTED_NAMES = ("huber", "huber_delta_1.25", "huber_scaled", "thresholds",
                 "behind_camera", "boundary", "rotated") + \
    tuple("nan_" + w for w in NAN_MAPS)


@functools.lru_cache(maxsize=None)
def crafted_case(name):
    """A crafted case by name, every regime in its `on` state. Cached: treat
    the arrays as read-only."""
    assert name in CRAFTED_NAMES
    if name.startswith("nan_"):
        return nan_planted(name[4:])
    return {"huber": huber_zones,
            "huber_delta_1.25": lambda: huber_zones(delta=1.25),
            "huber_scaled": lambda: huber_zones(scale=1 / 0.707),
            "thresholds": thresholds, "behind_camera": behind_camera,
            "boundary": boundary, "rotated": rotated}[name]()


# ---------------------------------------------------------------------------
# reduction geometry
# ---------------------------------------------------------------------------
# rows x cols: 1, 63..65, 255..257 pixels (one workgroup, idle lanes and
# waves), 65 535..65 537 (the 256-workgroup cap, first strided lane), 131 406
# (every lane strides twice, some a third time), cols = 1 and rows = 1.
REDUCTION_SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16),
                    (257, 1), (255, 257), (256, 256), (1, 65537), (65537, 1),
                    (363, 362))


def reduction_case(rows, cols, seed=0):
    """Seeded random float32 maps, identity T, target = source + a small
    offset, about half the source vertices NaN. Every other pixel projects
    onto itself with a residual far below trunc, so the inlier count of all
    three methods and of the information matrix is `mask.sum()`."""
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    f = np.float32
    n = rows * cols
    focal = float(max(rows, cols, 32))
    K = np.array([[focal, 0, (cols - 1) / 2], [0, focal, (rows - 1) / 2],
                  [0, 0, 1.0]])
    sd = rng.uniform(1.0, 2.0, (rows, cols)).astype(f)
    td = (sd + rng.uniform(-0.02, 0.02, (rows, cols))).astype(f)
    mask = rng.random((rows, cols)) < 0.5
    if n > 1:       # strictly between 0 and n
        mask.flat[0], mask.flat[n - 1] = True, False
    else:
        mask[:] = True
    sv = orc.create_vertex_map(sd, K, NAN)
    sv[~mask] = NAN
    nrm = rng.uniform(-1, 1, (rows, cols, 3)).astype(f)
    L = dict(K=K, T=np.eye(4), source_vertex=sv,
             target_vertex=orc.create_vertex_map(td, K, NAN),
             target_normal=nrm, source_depth=sd, target_depth=td,
             source_intensity=rng.random((rows, cols)).astype(f),
             target_intensity=rng.random((rows, cols)).astype(f),
             target_depth_dx=rng.uniform(-1, 1, (rows, cols)).astype(f),
             target_depth_dy=rng.uniform(-1, 1, (rows, cols)).astype(f),
             target_intensity_dx=rng.uniform(-1, 1, (rows, cols)).astype(f),
             target_intensity_dy=rng.uniform(-1, 1, (rows, cols)).astype(f))
    return _case(L, 0.5, 0.01, 0.1, 0.25, exact=False, mask=mask)


def stride_probe():
    """1 x 65537 point-to-plane input that pins which pixels share a lane in
    the strided regime: 256 workgroups of 256 lanes, so pixel 65536 is the
    second element of the lane that holds pixel 0, and pixel 256 is alone in
    its workgroup. All other source vertices are NaN. The (nx, ny) term of
    J^T J is 2^53 at pixel 0 and 1 at the other two: 2^53 + 1 rounds back to
    2^53 (ties to even) both inside the lane and in the final pass, so the
    sum is 2^53, as is the oracle's sequential one. Were the two small terms
    to meet first (any other lane assignment that pairs them), their 2 would
    survive: 2^53 + 2."""
    rows, cols = 1, 65537
    K = np.array([[65536.0, 0, 32768.0], [0, 65536.0, 0.0], [0, 0, 1.0]])
    u, v = _grid(rows, cols)
    sv = _vertex(u, v, 2.0, K)
    keep = np.zeros((rows, cols), bool)
    keep[0, [0, 256, 65536]] = True
    sv[~keep] = NAN
    tv = _vertex(u, v, 2.0, K)
    tv[..., 2] = 2.25
    tn = np.zeros((rows, cols, 3), np.float32)
    tn[..., :] = (1.0, 1.0, -1.0)
    tn[0, 0] = (2.0 ** 27, 2.0 ** 26, -1.0)
    L = dict(K=K, T=np.eye(4), source_vertex=sv, target_vertex=tv,
             target_normal=tn)
    return _case(L, 0.5, 0.125, 0.125, 0.5)


def sums_tolerance(want, n, delta_trunc):
    """Bound on |float64 sum in one order - float64 sum in another| of the
    same n float32 terms: 2 n 2^-53 sum|term|, with Cauchy-Schwarz
    sum|J_j J_k| <= sqrt(A_jj A_kk), sum|J_j d| <= sqrt(A_jj count) max|d|
    and max|d| <= max(delta, trunc). `want`: the oracle's 29 sums."""
    c = 2.0 * n * 2.0 ** -53
    diag = [want[j * (j + 1) // 2 + j] for j in range(6)]
    tol = np.zeros(29)
    i = 0
    for j in range(6):
        for k in range(j + 1):
            tol[i] = c * np.sqrt(diag[j] * diag[k])
            i += 1
        tol[21 + j] = c * np.sqrt(diag[j] * want[28]) * delta_trunc
    tol[27] = c * want[27]
    return tol


# ---------------------------------------------------------------------------
# images below the footprint of the stencils
# ---------------------------------------------------------------------------
SMALL_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (2, 3), (3, 2), (5, 33),
                (9, 65))
LEVEL_SHAPES = ((1, 1), (2, 2), (7, 31), (8, 32), (9, 33), (16, 64), (17, 65))


def small_images(rows, cols, seed=0):
    """(random float32 image, depth image in metres with NaN holes)."""
    rng = np.random.default_rng(seed + 100 * rows + cols)
    img = rng.random((rows, cols)).astype(np.float32)
    depth = rng.uniform(0.5, 2.5, (rows, cols)).astype(np.float32)
    if min(rows, cols) >= 5:
        depth[rng.random((rows, cols)) < 0.05] = NAN
        depth.flat[rows * cols // 2] = NAN
    elif rows * cols >= 6:
        # below the 5 x 5 footprint: one hole in a corner, which the
        # bilateral disc (dx^2 + dy^2 <= 4) of the far pixels does not reach
        depth.flat[0] = NAN
    return img, depth


def small_intrinsics(rows, cols):
    return np.array([[50.0, 0, (cols - 1) / 2], [0, 50.0, (rows - 1) / 2],
                     [0, 0, 1.0]])


def level_holes(rows, cols):
    """Sparse holes next to, not across, the borders of the 32 x 8 tiles of
    the fused level kernel. The 5 x 5 bilateral disc spreads a NaN two pixels
    each way, so a hole three or more pixels from the border pair (rows 7|8,
    columns 31|32 of a tile) leaves the smoothed depths that cross the LDS
    halo finite."""
    u, v = _grid(rows, cols)
    u, v = u.astype(int), v.astype(int)
    near_cols = np.isin(u % 32, (29, 30, 31, 0, 1, 2))
    near_rows = np.isin(v % 8, (5, 6, 7, 0, 1, 2))
    return (np.isin(v % 8, (3, 4)) & (u % 7 == 2) & ~near_cols) | \
        (np.isin(u % 32, (28, 3)) & (v % 5 == 1) & ~near_rows)


def level_pair(rows, cols, seed=0):
    """Source and target depth (metres, NaN holes at level_holes) of one
    pyramid level: a smooth surface plus millimetre noise."""
    rng = np.random.default_rng(seed + 100 * rows + cols)
    u, v = _grid(rows, cols)
    out = []
    for k in range(2):
        d = 1.5 + 0.3 * np.sin((u + 3 * k) / 11) + 0.2 * np.cos(v / 5) + \
            rng.normal(0, 0.002, (rows, cols))
        d = d.astype(np.float32)
        if rows * cols > 4:
            d[level_holes(rows, cols)] = NAN
        out.append(d)
    return out[0], out[1]
