"""PointCloud::ComputeMetrics and the nearest-point distances on a
voxel-down-sampled synthetic room (tools/bench_pointcloud_segment.py's),
Float32 -> profiles/pointcloud_metrics_bench.json.

Cloud 1 is the room at about 100 k and about 1 M points; cloud 2 is a copy,
jittered by half a voxel and shifted by three voxels. The `outliers` cases add
0.1 % points far outside the room to cloud 2, so that the second pass runs.

  metrics    the whole compute_metrics call (Chamfer, Hausdorff, FScore at three
             radii): two searches, two reductions, the host waits
  nearest    the two o3dmi_pointcloud_nearest_distance calls
  knn1       what a caller had before: o3dmi_nns_knn_search with knn = 1 in both
             directions and the torch chain on its output (sqrt, mean, max, one
             comparison and sum per radius, .item() each). The distances are
             asserted to be the same bits, the indices to be equal.

Warm, event-timed medians of 10 with the host waits included. Both sides are
this project's code: a record, not a pass mark.

Kernel times come from runs of their own, one case per process:

    python tools/bench_pointcloud_metrics.py
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o <case> -- \\
        python tools/bench_pointcloud_metrics.py --case <case> --reps 3
    python tools/bench_pointcloud_metrics.py --kernel-trace <case>=<csv> ...

The comparison that matters per direction, kernel time against kernel time on
the same index: NearestGroupKernel (16 lanes per query) against the first-pass
launch of KnnSearchKernel<TopKOut> with knn = 1 (a wave per query)."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from open3d_amd import pointcloud, registration  # noqa: E402
from bench_pointcloud_segment import VOXEL, room  # noqa: E402

RADII = (VOXEL, 2 * VOXEL, 5 * VOXEL)
METRICS = (pointcloud.Metric.ChamferDistance,
           pointcloud.Metric.HausdorffDistance, pointcloud.Metric.FScore)
KERNELS = ("NearestGroupKernel", "KnnSearchKernel", "MetricsElementKernel",
           "RunSumKernel", "BoundsKernel", "CountOccupiedKernel", "CountKernel",
           "AssignRangesKernel", "ScatterKernel", "FiniteCheckKernel")
CASES = {"100k": (100000, False), "100k_outliers": (100000, True),
         "1m": (1000000, False), "1m_outliers": (1000000, True)}


def clouds(n_target, outliers):
    p1 = room(int(n_target / 1.8))  # the room gives about 1.8 x its target
    rng = np.random.RandomState(11)
    n = p1.shape[0]
    p2 = p1.cpu().numpy() + rng.normal(scale=VOXEL / 2, size=(n, 3)).astype(
        np.float32) + np.array([3 * VOXEL, 0, 0], np.float32)
    if outliers:
        side = float(p1.max() - p1.min())
        far = rng.uniform(5 * side, 10 * side, (max(n // 1000, 1), 3))
        p2 = np.concatenate([p2, far.astype(np.float32)])
    return p1, torch.from_numpy(p2.astype(np.float32)).cuda().contiguous()


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


def knn1_chain(p1, p2):
    """The parent commit's way to the same numbers."""
    out = {}
    for name, (q, t) in (("12", (p1, p2)), ("21", (p2, p1))):
        idx, d2 = registration.knn_search(t, q, 1)
        d = d2[:, 0].sqrt()
        out[name] = dict(d=d, idx=idx[:, 0], mean=d.mean().item(),
                         max=d.max().item(),
                         counts=[(d < r).sum().item() for r in RADII])
    return out


def run_case(name, reps, compare):
    n_target, outliers = CASES[name]
    p1, p2 = clouds(n_target, outliers)
    a1, a2 = {"positions": p1}, {"positions": p2}
    out = dict(points1=p1.shape[0], points2=p2.shape[0], outliers=outliers)
    keep = {}

    def metrics():
        keep["m"] = pointcloud.compute_metrics(a1, a2, METRICS, RADII,
                                               return_raw=True)

    def nearest():
        keep["12"] = pointcloud.compute_point_cloud_distance(a1, a2, True)
        keep["21"] = pointcloud.compute_point_cloud_distance(a2, a1, True)

    out["metrics_call"] = timed(metrics, reps)
    out["nearest_distance_calls"] = timed(nearest, reps)
    values, raw = keep["m"]
    out["values"] = values.tolist()
    out["second_pass_queries"] = raw["second_pass_queries"]
    if not compare:
        knn1_chain(p1, p2)  # a kernel-trace run sees both sides
        return out
    out["knn1_and_torch_chain"] = timed(
        lambda: keep.__setitem__("k", knn1_chain(p1, p2)), reps)
    for d in ("12", "21"):
        dist, idx = keep[d]
        # float32 -> float64 sqrt -> float32 is the correctly rounded root
        idx_k, d2_k = registration.knn_search(p2 if d == "12" else p1,
                                              p1 if d == "12" else p2, 1)
        want = d2_k[:, 0].double().sqrt().float()
        assert torch.equal(dist.view(torch.int32), want.view(torch.int32)), d
        assert torch.equal(idx, idx_k[:, 0]), d
        out["torch_float32_sqrt_same_bits_" + d] = torch.equal(
            keep["k"][d]["d"].view(torch.int32), dist.view(torch.int32))
    out["same_bits_as_knn1"] = True
    out["speedup_metrics_vs_knn1_chain"] = (
        out["knn1_and_torch_chain"]["median_ms"] /
        out["metrics_call"]["median_ms"])
    return out


def kernel_averages(path):
    """Per kernel and grid size of a kernel-trace CSV: launches and duration
    (us). The first pass of a search is the launch with the largest grid."""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            short = next((k for k in KERNELS if k + "<" in name
                          or k + "(" in name or name.endswith(k)), None)
            if short is None:
                continue
            if short == "KnnSearchKernel":
                short += "<NearestOut>" if "NearestOut" in name else (
                    "<TopKOut>" if "TopKOut" in name else "<other>")
            grid = row.get("Grid_Size") or row.get("Grid_Size_X") or "?"
            ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            groups.setdefault(short, {}).setdefault(str(grid), []).append(ns)
    out = {}
    for k, by_grid in groups.items():
        out[k] = {g: {"launches": len(v),
                      "avg_us": round(sum(v) / len(v) / 1e3, 2),
                      "min_us": round(min(v) / 1e3, 2),
                      "max_us": round(max(v) / 1e3, 2)}
                  for g, v in by_grid.items()}

    def first_pass(short):
        by_grid = out.get(short)
        if not by_grid:
            return None
        g = max(by_grid, key=lambda s: int(s) if s.isdigit() else -1)
        return by_grid[g]["avg_us"]

    out["first_pass_per_direction_us"] = dict(
        lane_group=first_pass("NearestGroupKernel"),
        knn_topk_knn1=first_pass("KnnSearchKernel<TopKOut>"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--case")
    ap.add_argument("--kernel-trace", nargs="*", default=[],
                    metavar="CASE=CSV")
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "pointcloud_metrics_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        result = json.load(open(a.out))
        for item in a.kernel_trace:
            case, path = item.split("=", 1)
            result["cases"][case]["kernels"] = kernel_averages(path)
        json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud_metrics needs the GPU")
    if a.case:  # the body of a kernel-trace run: nothing is written
        run_case(a.case, a.reps, False)
        return 0
    result = dict(device=torch.cuda.get_device_name(0), dtype="Float32",
                  voxel=VOXEL, radii=list(RADII),
                  comparison="o3dmi_nns_knn_search with knn = 1 in both "
                             "directions + torch sqrt / mean / max / "
                             "comparisons",
                  cases={k: run_case(k, a.reps, True) for k in CASES})
    json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
