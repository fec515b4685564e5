"""PointCloud::GetOrientedBoundingBox (MINIMAL_APPROX, PCA) and
GetOrientedBoundingEllipsoid -> profiles/bounding_volume_bench.json.

The shapes of tools/bench_convex_hull.py: points uniform in the unit cube at
~100 k and ~1 M (few hull vertices), ~20 k points ON the unit sphere (every
point is a vertex) and the synthetic room. Every call starts with the convex
hull, which dominates (docs/pointcloud_convex_hull.md), so the hull is timed
apart and each call is reported as its median and as "rest" = its median less
the hull's. MINIMAL_APPROX is run with lane = one triangle (the public call)
and split over vertex slices (--split, the internal call); the ellipsoid in
its resident and its streamed form wherever the hull fits the resident form.
The numpy oracle
(tests/_bounding_volume_oracle.py) runs on the host beside them, on the hull
the device returned, where triangles x vertices stays below --host-limit.

    python tools/bench_bounding_volume.py
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from open3d_amd import _lib, pointcloud  # noqa: E402
from open3d_amd.core import TORCH_TO_O3DMI, stream  # noqa: E402
from bench_pointcloud_segment import room, timed  # noqa: E402
import _bounding_volume_oracle as orc  # noqa: E402


def stats():
    s = (C.c_int64 * 5)()
    v = (C.c_double * 16)()
    _lib.check(_lib.lib().o3dmi_internal_bounding_volume_stats(s, v), "stats")
    return dict(vertices=s[0], triangles=s[1], iterations=s[2], form=s[3],
                winner=s[4])


def with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def case(name, p, reps, split, host_limit):
    cloud = {"positions": p}
    capacity = _lib.lib().o3dmi_internal_obe_resident_capacity()
    hull = timed(lambda: pointcloud.compute_convex_hull(cloud), reps)
    out = dict(case=name, points=int(p.shape[0]), dtype=str(p.dtype),
               hull=hull)

    def run(key, fn):
        fn()
        t = timed(fn, reps)
        t["rest_ms"] = t["median_ms"] - hull["median_ms"]
        out[key] = dict(**stats(), **t)

    def box(method):
        return lambda: pointcloud.get_oriented_bounding_box(cloud,
                                                            method=method)

    def ellipsoid():
        return pointcloud.get_oriented_bounding_ellipsoid(cloud)

    def box_split():
        outs = [(C.c_double * k)() for k in (3, 9, 3)]
        _lib.check(_lib.lib().o3dmi_internal_pointcloud_obb_minimal_approx(
            _lib.ptr(p), p.shape[0], TORCH_TO_O3DMI[p.dtype], split, *outs,
            stream()), "obb_minimal_approx")

    run("minimal_approx_lane_per_triangle", box("minimal_approx"))
    run("minimal_approx_split_%d" % split, box_split)
    run("pca", box("pca"))
    v = out["pca"]["vertices"]
    if v <= capacity:
        run("ellipsoid_resident",
            lambda: with_env("O3DMI_OBE_FORM", "resident", ellipsoid))
    run("ellipsoid_streamed",
        lambda: with_env("O3DMI_OBE_FORM", "streamed", ellipsoid))
    out["vertices"], out["triangles"] = v, out["pca"]["triangles"]
    if v * out["triangles"] <= host_limit:
        mesh = pointcloud.compute_convex_hull(cloud)
        X = mesh["positions"].double().cpu().numpy()
        tri = mesh["indices"].cpu().numpy().astype(np.int64)
        out["host_oracle_ms"] = dict(
            minimal_approx=host_ms(lambda: orc.minimal_approx(X, tri)),
            pca=host_ms(lambda: orc.pca(X)),
            ellipsoid=host_ms(lambda: orc.ellipsoid(X)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--sphere", type=int, default=20000)
    ap.add_argument("--room", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--split", type=int, default=8)
    ap.add_argument("--host-limit", type=int, default=50000000,
                    help="no host oracle above this many triangles x vertices")
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "bounding_volume_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bounding_volume: no GPU; nothing is measured "
                         "without one")
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               resident_capacity=int(
                   _lib.lib().o3dmi_internal_obe_resident_capacity()),
               cases=[])

    def done(c):
        res["cases"].append(c)
        print(json.dumps(c), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def go(name, pts):
        done(case(name, pts, args.reps, args.split, args.host_limit))

    for n in args.sizes:
        go("cube", torch.from_numpy(rng.random((n, 3))).cuda())
    if args.sphere:
        g = rng.standard_normal((args.sphere, 3))
        go("sphere", torch.from_numpy(
            g / np.linalg.norm(g, axis=1, keepdims=True)).cuda())
    if args.room:
        go("room", room(args.room))


if __name__ == "__main__":
    main()
