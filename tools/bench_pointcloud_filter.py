"""PointCloud filters on voxel-down-sampled surfaces of about 100 k and 1 M
Float32 points -> profiles/pointcloud_filter_bench.json. Warm, event-timed
medians, host waits included.

  (a) remove_statistical_outliers(20, 2.0), against the same mask assembled
      from o3dmi_nns_knn_search ({N,20} rows) + torch sqrt / mean / std / le
      and a torch boolean gather per attribute
  (b) remove_radius_outliers(16, 5 voxels)
  (c) select_by_mask of positions + normals + uint8 colours at 50 % kept, as a
      fraction of the HBM time of its own read + write bytes
  (d) remove_duplicated_points at 0 % and 50 % duplicates

    python tools/bench_pointcloud_filter.py [--sizes 150000 1500000] [--reps 9]
    rocprofv3 --kernel-trace --stats -- python tools/bench_pointcloud_filter.py --only a
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from open3d_amd import pointcloud, registration, synthetic  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
VOXEL = 0.01


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def chain_statistical(cloud, k, ratio):
    p = cloud["positions"]
    _, d2 = registration.knn_search(p, p, k)
    avg = d2.sqrt().mean(1)
    mean = avg.mean().double().item()
    c = avg - mean
    sq = (c * c).sum().double().item()
    thr = mean + ratio * (sq / (avg.shape[0] - 1)) ** 0.5
    mask = avg <= thr
    return {name: t[mask] for name, t in cloud.items()}, mask


def bench_size(n_sample, reps, only):
    pair = synthetic.make_icp_pair(1000, n_sample, seed=1)
    p, nrm = registration.voxel_down_sample(
        torch.from_numpy(pair["target"]).cuda(),
        torch.from_numpy(pair["target_normals"]).cuda(), VOXEL)
    n = p.shape[0]
    col = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device="cuda")
    cloud = {"positions": p, "normals": nrm, "colors": col}
    out = dict(points=n, voxel=VOXEL)
    if "a" in only:
        fused = timed(lambda: pointcloud.remove_statistical_outliers(
            cloud, 20, 2.0), reps)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        chain = timed(lambda: chain_statistical(cloud, 20, 2.0), reps)
        chain_peak = torch.cuda.max_memory_allocated() - base
        (_, m1) = pointcloud.remove_statistical_outliers(cloud, 20, 2.0)
        (_, m2) = chain_statistical(cloud, 20, 2.0)
        out["statistical"] = dict(
            fused=fused, chain=chain, kept=int(m1.sum()),
            mask_bits_differing_from_chain=int((m1 != m2).sum()),
            chain_peak_torch_bytes=int(chain_peak),
            chain_neighbour_table_bytes=n * 20 * 8,
            fused_scratch_bytes_beyond_index=n * 4 + n + 12 * n)
    if "b" in only:
        out["radius"] = dict(
            count_then_threshold=timed(
                lambda: pointcloud.remove_radius_outliers(cloud, 16,
                                                          5 * VOXEL), reps),
            early_out_variant="not built")
    if "c" in only:
        mask = torch.rand(n, device="cuda") < 0.5
        t = timed(lambda: pointcloud.select_by_mask(cloud, mask), reps)
        kept = int(mask.sum())
        moved = n * (27 + 1) + kept * 27 + n * (4 + 8) * 2
        t["bytes_moved_model"] = moved
        t["hbm_time_ms"] = moved / HBM_BYTES_PER_S * 1e3
        t["fraction_of_hbm_rate"] = t["hbm_time_ms"] / t["median_ms"]
        out["select_by_mask"] = t
    if "d" in only:
        half = torch.cat([p[:n // 2], p[:n - n // 2]])
        half = half[torch.randperm(n, device="cuda")].contiguous()
        out["duplicated"] = dict(
            none=timed(lambda: pointcloud.remove_duplicated_points(
                {"positions": p}), reps),
            half=timed(lambda: pointcloud.remove_duplicated_points(
                {"positions": half}), reps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+",
                    default=[150000, 1500000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "pointcloud_filter_bench.json"))
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32",
               reps=args.reps,
               cases=[bench_size(s, args.reps, args.only)
                      for s in args.sizes])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
