"""TriangleMesh topology and intersection queries on one MI355X ->
profiles/trianglemesh_topology_bench.json.

    python tools/bench_trianglemesh_topology.py [--out profiles/...json]
                                                [--radial 1024 --tubular 512]

Input: a closed torus made in numpy (major radius 1, minor radius 0.4),
radial x tubular quads of two triangles, 2^20 triangles by default, Float32
positions and Int32 indices; for is_intersecting a second copy linked through
the first. Warm, the median of 10 event-timed calls each, every call with its
range check, its pool allocations and its final wait:
  * euler_poincare_characteristic, is_edge_manifold (both flags),
    get_non_manifold_vertices (count, then fill), is_orientable,
    orient_triangles (half of the triangles flipped first);
  * get_self_intersecting_triangles (count, then fill), is_self_intersecting,
    is_intersecting, is_watertight, get_volume;
  * the visit counts of the self-intersection traversal: inner nodes opened
    and exact pair tests run, per triangle. The second is the number that shows
    the broad phase at work: upstream's loop runs m / 2 of them per triangle.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_trianglemesh as bt  # noqa: E402
from open3d_amd import _lib  # noqa: E402
from open3d_amd import trianglemesh as tm  # noqa: E402


def torus(radial, tubular, major=1.0, minor=0.4):
    u = 2 * np.pi * np.arange(radial) / radial
    w = 2 * np.pi * np.arange(tubular) / tubular
    r = major + minor * np.cos(w)[None, :]
    p = np.stack([r * np.cos(u)[:, None], r * np.sin(u)[:, None],
                  np.broadcast_to(minor * np.sin(w)[None, :],
                                  (radial, tubular))], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(radial), np.arange(tubular), indexing="ij")
    i1, j1 = (i + 1) % radial, (j + 1) % tubular
    a, b = i * tubular + j, i1 * tubular + j
    c, d = i1 * tubular + j1, i * tubular + j1
    t = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)],
                 2).reshape(-1, 3)
    return p.astype(np.float32), t.astype(np.int32)


def visits(mesh, kind):
    p, t = mesh["positions"], mesh["indices"]
    n = C.c_int64(0)
    v = (C.c_uint64 * 2)(0, 0)
    _lib.check(_lib.lib().o3dmi_internal_trianglemesh_self_intersections(
        _lib.ptr(p), p.shape[0], _lib.F32, _lib.ptr(t), t.shape[0], _lib.I32,
        kind, C.byref(n), v, None), "self_intersections")
    m = float(t.shape[0])
    return dict(pairs=n.value, inner_nodes_opened_per_triangle=v[0] / m,
                exact_pair_tests_per_triangle=v[1] / m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "trianglemesh_topology_bench.json"))
    ap.add_argument("--radial", type=int, default=1024)
    ap.add_argument("--tubular", type=int, default=512)
    a = ap.parse_args()
    p, t = torus(a.radial, a.tubular)
    mesh = {"positions": torch.from_numpy(p).cuda(),
            "indices": torch.from_numpy(t).cuda()}
    # the same torus turned into the plane y = 0 and moved through the hole
    q = p[:, [0, 2, 1]] + np.array([1.0, 0.0, 0.0], np.float32)
    other = {"positions": torch.from_numpy(np.ascontiguousarray(q)).cuda(),
             "indices": mesh["indices"]}
    far = {"positions": other["positions"] + 10.0, "indices": mesh["indices"]}
    flipped = t.copy()
    flipped[1::2] = flipped[1::2][:, [0, 2, 1]]
    mixed = {"positions": mesh["positions"],
             "indices": torch.from_numpy(flipped).cuda()}
    legs = {
        "euler_poincare_characteristic":
            lambda: tm.euler_poincare_characteristic(mesh),
        "is_edge_manifold": lambda: tm.is_edge_manifold(mesh, True),
        "is_edge_manifold_no_boundary":
            lambda: tm.is_edge_manifold(mesh, False),
        "get_non_manifold_vertices":
            lambda: tm.get_non_manifold_vertices(mesh).shape[0],
        "is_orientable": lambda: tm.is_orientable(mesh),
        "orient_triangles_half_flipped":
            lambda: tm.orient_triangles(mixed)[1],
        "get_self_intersecting_triangles":
            lambda: tm.get_self_intersecting_triangles(mesh).shape[0],
        "is_self_intersecting": lambda: tm.is_self_intersecting(mesh),
        "is_intersecting_linked": lambda: tm.is_intersecting(mesh, other),
        "is_intersecting_far_boxes": lambda: tm.is_intersecting(mesh, far),
        "is_watertight": lambda: tm.is_watertight(mesh),
        "get_volume": lambda: tm.get_volume(mesh),
    }
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32/int32",
               mesh="torus %d x %d" % (a.radial, a.tubular),
               vertices=int(p.shape[0]), triangles=int(t.shape[0]),
               calls=bt.CALLS, timing="median of event-timed calls, ms",
               torus_volume=2 * math.pi ** 2 * 0.4 ** 2)
    out = {}
    for name, fn in legs.items():
        def run():
            out["value"] = fn()
        ms, _ = bt.timed(run)
        value = out["value"]
        res[name] = {"ms": ms, "value": value if isinstance(
            value, (bool, int, float)) else str(value)}
    res["self_intersection_visits"] = visits(mesh, 0)
    res["is_self_intersecting_visits"] = visits(mesh, 1)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
