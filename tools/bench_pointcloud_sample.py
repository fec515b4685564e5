"""PointCloud::FarthestPointDownSample on a voxel-down-sampled synthetic room
(tools/bench_pointcloud_segment.py's), Float32, 1024 samples
-> profiles/pointcloud_sample_bench.json.

  resident   one launch for all samples: about 10 k points and at the capacity C
  streamed   one launch per sample: at C, about 100 k and about 1 M points
  torch      beside each, the chain a seam-by-seam port of upstream's tensor
             loop runs on the same device: subtract, square, row sum, minimum,
             arg-max, .item() per sample. The index sets are compared.
  crossover  both forms at a ladder of sizes up to C (256 samples), alternating
             in one process: the two numbers that decide where form 0 switches

Warm, event-timed medians of 10 with the host waits included; per-sample cost
= call time / samples. Both sides are this project's code: a record, not a
pass mark.

Streamed-form bound (MI355X): a sample reads 3 coordinates and dist and writes
dist, n (3 + 2) sizeof(dtype) bytes, against the cadence of dependent launches
on one stream. At 1 M Float32 points that is 20 MB, 2.5 us at 8 TB/s.

Kernel times come from runs of their own, one case per process:

    python tools/bench_pointcloud_sample.py
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o <case> -- \\
        python tools/bench_pointcloud_sample.py --case <case> --reps 3
    python tools/bench_pointcloud_sample.py --kernel-trace <case>=<csv> ...
"""
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

from open3d_amd import _lib, pointcloud  # noqa: E402
from bench_pointcloud_segment import room  # noqa: E402

SAMPLES = 1024
LADDER_SAMPLES = 256
HBM_BYTES_PER_S = 8e12
KERNELS = ("FarthestResidentKernel", "FarthestStreamKernel",
           "FarthestStreamSetupKernel", "FiniteCheckKernel")


def capacity():
    return _lib.lib().o3dmi_pointcloud_farthest_point_capacity(_lib.F32)


def cloud(n):
    """Exactly n points of the room: a seeded subset of a larger one."""
    target = n
    p = room(target)
    while p.shape[0] < n:  # the room gives about 1.8 x its target
        target = int(target * 1.5) + 1000
        p = room(target)
    keep = np.random.RandomState(7).permutation(p.shape[0])[:n]
    return p[torch.from_numpy(np.sort(keep)).cuda()].contiguous()


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


def torch_chain(p, k, start=0):
    """Upstream's loop (t/geometry/PointCloud.cpp:628-646) op for op."""
    dist = torch.full((p.shape[0],), float("inf"), dtype=p.dtype,
                      device=p.device)
    order = []
    sel = start
    for _ in range(k):
        order.append(sel)
        diff = p - p[sel]
        d = (diff * diff).sum(1)
        dist = torch.minimum(d, dist)
        sel = dist.argmax(0).item()
    return order


def cases():
    c = capacity()
    return {
        "resident_10k": (10000, 1),
        "resident_capacity": (c, 1),
        "streamed_capacity": (c, 2),
        "streamed_100k": (100000, 2),
        "streamed_1m": (1000000, 2),
    }


def run_case(name, reps, with_torch):
    n, form = cases()[name]
    p = cloud(n)
    out = dict(points=n, samples=SAMPLES, form=form)
    order = []

    def ours():
        order[:] = [pointcloud.farthest_point_order(p, SAMPLES, 0, form)]

    t = timed(ours, reps)
    out["call"] = t
    out["per_sample_us"] = t["median_ms"] * 1e3 / SAMPLES
    if form == 2:
        nbytes = n * (3 + 2) * 4
        out["bytes_per_sample"] = nbytes
        out["hbm_bound_per_sample_us"] = nbytes / HBM_BYTES_PER_S * 1e6
        out["achieved_bytes_per_s"] = nbytes / (out["per_sample_us"] * 1e-6)
    if with_torch:
        ref = []

        def chain():
            ref[:] = [torch_chain(p, SAMPLES)]

        tt = timed(chain, max(3, reps // 3))
        got = order[0].cpu().tolist()
        out["torch_chain"] = dict(
            call=tt, per_sample_us=tt["median_ms"] * 1e3 / SAMPLES,
            launches_per_sample=6, host_waits_per_sample=1,
            index_sets_equal=set(got) == set(ref[0]),
            orders_equal=got == ref[0],
            speedup=tt["median_ms"] / t["median_ms"])
    return out


def ladder(reps):
    """Both forms at sizes up to C, alternating call by call."""
    rows = []
    c = capacity()
    for n in (1024, 4096, 10000, 20000, c):
        p = cloud(n)
        ms = {1: [], 2: []}
        same = True
        for form in (1, 2):
            pointcloud.farthest_point_order(p, LADDER_SAMPLES, 0, form)
        for _ in range(reps):
            got = {}
            for form in (1, 2):
                ms[form].append(_once(lambda: got.__setitem__(
                    form, pointcloud.farthest_point_order(
                        p, LADDER_SAMPLES, 0, form))))
            same = same and torch.equal(got[1], got[2])
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        rows.append(dict(points=n, samples=LADDER_SAMPLES,
                         resident_per_sample_us=med[1] * 1e3 / LADDER_SAMPLES,
                         streamed_per_sample_us=med[2] * 1e3 / LADDER_SAMPLES,
                         same_bits=same))
    return rows


def kernel_averages(path):
    """Average duration (us) and launches per kernel of a kernel-trace CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            short = next((k for k in KERNELS if k + "<" in row["Kernel_Name"]
                          or k + "(" in row["Kernel_Name"]), None)
            if short is None:
                continue
            ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            out.setdefault(short, []).append(ns)
    return {k: {"launches": len(v), "avg_us": round(sum(v) / len(v) / 1e3, 2),
                "min_us": round(min(v) / 1e3, 2),
                "max_us": round(max(v) / 1e3, 2)} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--case")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--kernel-trace", nargs="*", default=[],
                    metavar="CASE=CSV")
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "pointcloud_sample_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        result = json.load(open(a.out))
        for item in a.kernel_trace:
            case, path = item.split("=", 1)
            result["cases"][case]["kernels"] = kernel_averages(path)
        json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud_sample needs the GPU")
    if a.case:  # the body of a kernel-trace run: nothing is written
        run_case(a.case, a.reps, False)
        return 0
    result = dict(device=torch.cuda.get_device_name(0), dtype="Float32",
                  capacity_float32=capacity(),
                  capacity_float64=_lib.lib()
                  .o3dmi_pointcloud_farthest_point_capacity(_lib.F64),
                  cases={k: run_case(k, a.reps, not a.no_torch)
                         for k in cases()},
                  crossover=ladder(a.reps))
    at_c = result["crossover"][-1]
    result["form_0_switch"] = dict(
        at_points=capacity(),
        resident_per_sample_us_at_capacity=at_c["resident_per_sample_us"],
        streamed_per_sample_us_at_capacity=at_c["streamed_per_sample_us"],
        resident_is_faster_at_capacity=at_c["resident_per_sample_us"] <
        at_c["streamed_per_sample_us"])
    json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
