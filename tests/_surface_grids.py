"""Synthetic TSDF blocks for the surface-extraction tests (point cloud and
triangle mesh), at any block resolution: a sphere whose surface crosses
block faces, edges and corners, over a cube of blocks with random holes
(some neighbours absent) and negative keys."""
import numpy as np


def sphere_blocks(res, wdt, with_color, seed=0, edge_values=False,
                  thresholds=(3.0, 10.0)):
    """-> (keys {n,3} int32, tsdf {n,R^3} float32, weight {n,R^3} wdt,
    color {n,R^3,3} wdt or None).

    The cube of blocks spans at least 12 voxels a side, so small resolutions
    still see several blocks across the surface; about a ninth of the blocks
    are dropped. Weights are 20 for most voxels and 0..11 for the rest.

    edge_values: near the surface (within a voxel), a tenth of the voxels
    get tsdf +0.0 and a tenth -0.0, and a fifth get a weight exactly equal
    to one of `thresholds`."""
    rng = np.random.default_rng(seed)
    m = max(3, -(-12 // res))
    lo = -(m // 2)
    keys = np.array([(i, j, k) for k in range(lo, lo + m)
                     for j in range(lo, lo + m) for i in range(lo, lo + m)],
                    np.int32)
    keep = max(1, len(keys) - len(keys) // 9)
    keys = keys[rng.permutation(len(keys))[:keep]]
    v = np.arange(res ** 3)
    X = keys[:, :1] * res + v % res
    Y = keys[:, 1:2] * res + (v // res) % res
    Z = keys[:, 2:] * res + v // (res * res)
    r = 1.1 * res * m / 3
    dist = np.sqrt((X - 0.3) ** 2 + (Y + 0.2) ** 2 + (Z - 0.1) ** 2) - r
    tsdf = (dist / res + 0.02 * rng.standard_normal(dist.shape)).astype(
        np.float32)
    w = rng.integers(0, 12, tsdf.shape)
    w[rng.random(tsdf.shape) < 0.9] = 20
    if edge_values:
        near = np.abs(dist) < 1.0
        u = rng.random(tsdf.shape)
        tsdf[near & (u < 0.1)] = np.float32(0.0)
        tsdf[near & (u >= 0.1) & (u < 0.2)] = np.float32(-0.0)
        at = near & (rng.random(tsdf.shape) < 0.2)
        w[at] = rng.choice(np.asarray(thresholds), int(at.sum()))
    weight = w.astype(wdt)
    color = rng.integers(0, 256, tsdf.shape + (3,)).astype(wdt) \
        if with_color else None
    return keys, tsdf, weight, color


def has_edge_values(tsdf, weight, thresholds):
    """The edge values sphere_blocks(edge_values=True) plants are present."""
    zero = tsdf == 0
    return (bool((zero & ~np.signbit(tsdf)).any()) and
            bool((zero & np.signbit(tsdf)).any()) and
            all(bool((weight == t).any()) for t in thresholds))
