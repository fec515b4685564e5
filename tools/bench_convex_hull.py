"""PointCloud::ComputeConvexHull and HiddenPointRemoval
-> profiles/convex_hull_bench.json.

  cube     the hull of points uniform in the unit cube, ~100 k and ~1 M: few
           hull vertices, the time is the first passes over the cloud
  sphere   the hull of ~100 k points ON the unit sphere: every point is a
           vertex, the worst case for rounds and cavity conflicts
  hpr      hidden_point_removal of the voxel-down-sampled synthetic room
           (tools/bench_pointcloud_segment.room) at ~100 k and ~1 M points,
           from a camera inside it at radius 100 x the room's diameter

Median of `reps` warm, event-timed calls with the host waits included (the
Python mirror: one native call at the bounds V <= n, T <= 2 n - 4). Beside each
time: the rounds of the call, how many were sweep rounds, the winners per
round and the candidates refused per round (o3dmi_internal_pointcloud_hull_
stats). If scipy imports, scipy.spatial.ConvexHull with "Qt" -- Qhull, the
library upstream calls on a host copy -- runs ONCE on the same float64 input on
the host beside it. Nobody measured any of this before: a record, not a pass
mark.

Kernel times come from a run of their own:

    python tools/bench_convex_hull.py
    rocprofv3 --kernel-trace --stats -d <dir> -- \\
        python tools/bench_convex_hull.py --reps 3 --no-host --out /dev/null
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
from bench_pointcloud_segment import room, timed  # noqa: E402
import _pointcloud_hull_oracle as orc  # noqa: E402


def stats():
    out = (C.c_int64 * 4)()
    _lib.check(_lib.lib().o3dmi_internal_pointcloud_hull_stats(out), "stats")
    rounds, sweeps, winners, refused = list(out)
    return dict(rounds=rounds, sweep_rounds=sweeps, winners=winners,
                winners_per_round=winners / max(rounds, 1),
                refused_per_round=refused / max(rounds, 1))


def qhull_ms(P):
    try:
        from scipy.spatial import ConvexHull
    except ImportError:
        return None
    t = time.perf_counter()
    hull = ConvexHull(P, qhull_options="Qt")
    return dict(ms=(time.perf_counter() - t) * 1e3,
                vertices=int(len(hull.vertices)))


def hull_case(name, pts, reps, host):
    cloud = {"positions": torch.from_numpy(pts).cuda()}
    mesh = pointcloud.compute_convex_hull(cloud)
    out = dict(case=name, points=len(pts), dtype=str(pts.dtype),
               vertices=int(mesh["positions"].shape[0]),
               triangles=int(mesh["indices"].shape[0]), **stats(),
               device=timed(lambda: pointcloud.compute_convex_hull(cloud),
                            reps))
    if host:
        out["host_qhull"] = qhull_ms(pts.astype(np.float64))
    return out


def hpr_case(n_target, reps, host):
    p = room(n_target)
    lo, hi = p.min(dim=0).values, p.max(dim=0).values
    diameter = float((hi - lo).norm())
    camera = (0.5 * (lo + hi)).double().cpu().tolist()
    radius = 100.0 * diameter
    cloud = {"positions": p}
    mesh, idx = pointcloud.hidden_point_removal(cloud, camera, radius)
    out = dict(case="hpr_room", points=int(p.shape[0]), dtype="float32",
               camera=camera, radius=radius, visible=int(idx.shape[0]),
               triangles=int(mesh["indices"].shape[0]), **stats(),
               device=timed(lambda: pointcloud.hidden_point_removal(
                   cloud, camera, radius), reps))
    if host:
        flipped = orc.flip(p.cpu().numpy().astype(np.float64), camera, radius)
        out["host_qhull"] = qhull_ms(np.concatenate([flipped,
                                                     np.zeros((1, 3))]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--sphere", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-limit", type=int, default=1000000,
                    help="no host Qhull run for a case aimed above this "
                         "many points")
    ap.add_argument("--cases", nargs="+", default=["cube", "sphere", "hpr"],
                    choices=["cube", "sphere", "hpr"])
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "convex_hull_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_convex_hull: no GPU; nothing is measured "
                         "without one")
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, cases=[])

    def done(case):
        """Every finished case is printed and the file rewritten: a long run
        leaves what it measured."""
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def host(points):
        return not args.no_host and points <= args.host_limit

    for n in args.sizes if "cube" in args.cases else []:
        done(hull_case("cube", rng.random((n, 3)), args.reps, host(n)))
    if "sphere" in args.cases:
        g = rng.standard_normal((args.sphere, 3))
        done(hull_case("sphere", g / np.linalg.norm(g, axis=1, keepdims=True),
                       args.reps, host(args.sphere)))
    for n in args.sizes if "hpr" in args.cases else []:
        done(hpr_case(n, args.reps, host(n)))


if __name__ == "__main__":
    main()
