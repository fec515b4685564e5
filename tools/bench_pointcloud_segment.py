"""PointCloud::ClusterDBSCAN and PointCloud::SegmentPlane on a voxel-down-
sampled synthetic room (floor, two walls, separate objects) of about 100 k and
1 M Float32 points -> profiles/pointcloud_segment_bench.json.

  dbscan    eps = 2.5 voxels, min_points 10
  segment   1000 iterations, ransac_n 3, threshold = 1 voxel; once at
            upstream's default probability (the walk ends early on the floor)
            and once at probability 1 (all 1000 hypotheses are scored)
  score     o3dmi_plane_score alone, 1024 planes: evaluations/s against the
            two bounds below

Warm, event-timed medians with the host waits included. Beside each: the same
operator through the numpy restatement on the host (tests/_pointcloud_segment_
oracle.py) -- what a device caller gets upstream, where both calls convert to
the legacy CPU cloud. Both sides are this project's code: a record, not a pass
mark. The host side of DBSCAN runs at the small size only (its neighbour sets
are quadratic), and host runs are single (seconds each).

Score kernel bounds (MI355X): every evaluation is 3 mul + 3 add + abs/compare
+ mul + add in float64 with no FMA, 9 VALU float64 issues per lane; the float64
VALU issues 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 3.93e13 lane-operations/s,
so 4.4e12 evaluations/s is the issue bound. Point traffic: a workgroup of 256
hypotheses reads a 512-point tile (6 KiB) for 131072 evaluations, 0.047
bytes/evaluation through the scalar cache -- three orders of magnitude below
what memory delivers, so the VALU bound is the one that can bind.

Kernel times come from a run of their own:

    python tools/bench_pointcloud_segment.py [--sizes 100000 1000000]
    rocprofv3 --kernel-trace --stats -d <dir> -- \\
        python tools/bench_pointcloud_segment.py --reps 3 --no-host --out /dev/null
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

from open3d_amd import _lib, pointcloud, registration  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

VOXEL = 0.01
EPS, MIN_POINTS = 2.5 * VOXEL, 10
THRESHOLD, RANSAC_N, ITERATIONS = VOXEL, 3, 1000
SCORE_PLANES = 1024
VALU_F64_LANE_OPS = 256 * 4 * 16 * 2.4e9
OPS_PER_EVALUATION = 9
TILE_BYTES_PER_EVALUATION = 512 * 12 / (256.0 * 512)


def room(n_target, seed=0):
    """Floor, two walls and eight separate boxes / balls, sampled densely and
    voxel-down-sampled; the room's extent is chosen for about n_target points
    at VOXEL."""
    rng = np.random.RandomState(seed)
    # surface area in voxels^2 ~ points: floor + 2 walls (0.6 high) + objects
    side = np.sqrt(n_target * VOXEL * VOXEL / 2.6)
    dense = int(n_target * 6)
    parts = []
    k = dense // 2
    parts.append(np.column_stack([rng.uniform(0, side, (k, 2)), np.zeros(k)]))
    k = dense // 6
    h = 0.6 * side
    parts.append(np.column_stack([rng.uniform(0, side, k), np.zeros(k),
                                  rng.uniform(0, h, k)]))
    parts.append(np.column_stack([np.zeros(k), rng.uniform(0, side, k),
                                  rng.uniform(0, h, k)]))
    k = dense // 48
    for j in range(8):
        c = np.array([(0.2 + 0.2 * (j % 4)) * side,
                      (0.3 + 0.4 * (j // 4)) * side, 0.25 * side])
        r = 0.06 * side
        if j % 2:
            v = rng.normal(size=(k, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
        else:
            v = rng.uniform(-1, 1, (k, 3))
            face = rng.randint(0, 3, k)
            v[np.arange(k), face] = np.sign(v[np.arange(k), face])
        parts.append(c + r * v)
    pts = np.vstack(parts).astype(np.float32)
    pts += rng.normal(scale=VOXEL / 10, size=pts.shape).astype(np.float32)
    p, _ = registration.voxel_down_sample(torch.from_numpy(pts).cuda(), None,
                                          VOXEL)
    return p.contiguous()


def _once(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = sorted(_once(fn) for _ in range(reps))
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def host_once(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def score_case(p, reps):
    n = p.shape[0]
    rng = np.random.RandomState(1)
    normals = rng.normal(size=(SCORE_PLANES, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    planes = torch.from_numpy(np.hstack(
        [normals, rng.uniform(-1, 0, (SCORE_PLANES, 1))])).cuda()
    counts = torch.empty(SCORE_PLANES, dtype=torch.int64, device="cuda")
    sums = torch.empty(SCORE_PLANES, dtype=torch.float64, device="cuda")

    def run():
        _lib.check(_lib.lib().o3dmi_plane_score(
            _lib.ptr(p), n, _lib.F32, _lib.ptr(planes), SCORE_PLANES,
            C.c_double(THRESHOLD), _lib.ptr(counts), _lib.ptr(sums),
            stream()), "plane_score")

    t = timed(run, reps)
    rate = SCORE_PLANES * n / (t["median_ms"] * 1e-3)
    bound = VALU_F64_LANE_OPS / OPS_PER_EVALUATION
    return dict(planes=SCORE_PLANES, call=t, evaluations_per_s=rate,
                valu_f64_issue_bound_evaluations_per_s=bound,
                fraction_of_valu_bound=rate / bound,
                point_bytes_per_s=rate * TILE_BYTES_PER_EVALUATION,
                binds="VALU float64 issue" if rate / bound > 0.5 else
                "neither bound is reached; the point traffic is far from "
                "binding, the VALU bound is the nearer one")


def bench_size(n_target, reps, host, host_dbscan_limit):
    import _pointcloud_segment_oracle as orc
    p = room(n_target)
    n = p.shape[0]
    cloud = {"positions": p}
    out = dict(points=n, voxel=VOXEL)

    labels, clusters, noise = pointcloud.cluster_dbscan(
        cloud, EPS, MIN_POINTS, return_counts=True)
    out["dbscan"] = dict(
        eps=EPS, min_points=MIN_POINTS, clusters=clusters, noise=noise,
        device=timed(lambda: pointcloud.cluster_dbscan(cloud, EPS, MIN_POINTS),
                     reps))
    out["segment"] = {}
    for name, prob in (("default_probability", 0.99999999),
                       ("probability_1", 1.0)):
        _, inl, info = pointcloud.segment_plane(
            cloud, THRESHOLD, RANSAC_N, ITERATIONS, prob, 0, return_info=True)
        out["segment"][name] = dict(
            inliers=int(inl.shape[0]), info=info,
            device=timed(lambda: pointcloud.segment_plane(
                cloud, THRESHOLD, RANSAC_N, ITERATIONS, prob, 0), reps))
    out["score"] = score_case(p, reps)

    if host:
        pts = p.cpu().numpy()
        if n <= host_dbscan_limit:
            want, ms = host_once(lambda: orc.cluster_dbscan(pts, EPS,
                                                            MIN_POINTS))
            out["dbscan"]["host_numpy_ms"] = ms
            out["dbscan"]["labels_differing"] = int(
                (want != labels.cpu().numpy()).sum())
        else:
            out["dbscan"]["host_numpy_ms"] = None  # not measured: quadratic
        for name, prob in (("default_probability", 0.99999999),
                           ("probability_1", 1.0)):
            want, ms = host_once(lambda: orc.segment_plane(
                pts, THRESHOLD, RANSAC_N, ITERATIONS, prob, 0, batch=256))
            seg = out["segment"][name]
            seg["host_numpy_ms"] = ms
            seg["same_best_iteration"] = (
                want["best_iteration"] == seg["info"]["best_iteration"])
            seg["same_inlier_count"] = len(want["inliers"]) == seg["inliers"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-dbscan-limit", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "pointcloud_segment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud_segment: no GPU; nothing is "
                         "measured without one")
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32",
               reps=args.reps,
               cases=[bench_size(s, args.reps, not args.no_host,
                                 args.host_dbscan_limit) for s in args.sizes])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
