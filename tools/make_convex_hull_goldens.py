"""Records tests/golden/convex_hull/*.npz from Qhull, the library upstream
calls: scipy.spatial.ConvexHull(points, qhull_options="Qt"), the options
upstream passes (Qhull.cpp). Each file holds the input, the canonicalised vertex
indices and triangles (tests/_pointcloud_hull_oracle.canonical) and, for
hidden-point removal, the camera and the radius.

    python tools/make_convex_hull_goldens.py

Every input is chosen so that Qhull alone decides nothing: no coplanar point,
F = 2 V - 4, and every point that is not a vertex of a facet lies below it by
at least 1e-9 of the cloud's extent, four orders of magnitude above the
library's eps. A seed that fails this is replaced, the condition is not
loosened."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pointcloud_hull_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "convex_hull")
MIN_MARGIN = 1e-9  # of the largest extent of the bounding box
CAMERA, RADIUS = (0.0, 0.0, 4.0), 400.0


def _cube(seed):
    return np.random.default_rng(seed).random((3000, 3))


def _sphere(seed):
    g = np.random.default_rng(seed).standard_normal((1500, 3))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def _bumpy(seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((3000, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return g * (1.0 + 0.05 * rng.random(3000))[:, None]


# name -> (points in their dtype, is hidden-point removal)
CASES = {
    "cube3000_s0_f64": lambda: (_cube(0), False),
    "cube3000_s1_f64": lambda: (_cube(1), False),
    "cube3000_s0_f32": lambda: (_cube(0).astype(np.float32), False),
    "cube3000_s1_f32": lambda: (_cube(1).astype(np.float32), False),
    "sphere1500_f64": lambda: (_sphere(2), False),
    "sphere1500_f32": lambda: (_sphere(2).astype(np.float32), False),
    "hpr_bumpy3000_f64": lambda: (_bumpy(3), True),
}


def qhull(P):
    """Qhull's hull of float64 P -> oriented triangles on point indices, after
    the condition above is asserted."""
    from scipy.spatial import ConvexHull
    hull = ConvexHull(P, qhull_options="Qt")
    assert len(hull.coplanar) == 0, "coplanar points"
    tris = hull.simplices.astype(np.int64)
    assert len(tris) == 2 * len(hull.vertices) - 4, "F != 2 V - 4"
    nrm, off = hull.equations[:, :3], hull.equations[:, 3]
    dist = P @ nrm.T + off  # {points, facets}, <= 0 inside
    dist[tris.T, np.arange(len(tris))[None, :]] = -np.inf
    extent = float((P.max(axis=0) - P.min(axis=0)).max())
    margin = float((-dist).min())
    assert margin >= MIN_MARGIN * extent, "margin %g" % (margin / extent)
    a, b, c = P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), nrm) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return tris


def record(name):
    """-> the arrays of golden `name`."""
    points, hpr = CASES[name]()
    P = points.astype(np.float64)
    out = {"points": points}
    if hpr:
        out["camera"] = np.array(CAMERA, np.float64)
        out["radius"] = np.float64(RADIUS)
        n = len(P)
        tris = qhull(np.concatenate([orc.flip(P, CAMERA, RADIUS),
                                     np.zeros((1, 3))]))
        tris = tris[(tris != n).all(axis=1)]
    else:
        tris = qhull(P)
    verts, t = orc.canonical(tris)
    out["point_indices"] = verts.astype(np.int64)
    out["triangles"] = t.astype(np.int64)
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        arrays = record(name)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print("%s: V = %d, T = %d, %d bytes" % (
            name, len(arrays["point_indices"]), len(arrays["triangles"]),
            os.path.getsize(path)))


if __name__ == "__main__":
    main()
