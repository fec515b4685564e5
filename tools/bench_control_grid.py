"""ControlGrid timings on the MI355X.

    python tools/bench_control_grid.py [--reps 20] [--out profiles/control_grid_bench.json]
    python tools/bench_control_grid.py --case cloud_1m --reps 5   # under a profiler
    python tools/bench_control_grid.py --kernel-trace cloud_1m=<kernel_trace.csv> ...

Cases: Parameterize + Deform of a cloud of 100 k and 1 M points (a 3 m box, 729
nodes), and the RGB-D Deform of a 640x480 and a 1280x720 synthetic frame, fused
against the seam-by-seam chain (unproject -> parameterize -> deform -> project)
on the same input. The first form records event times of whole calls (host
waits included, median of --reps); --case runs one case alone, which is what a
`rocprofv3 --kernel-trace --output-format csv` run wraps; --kernel-trace folds
the per-kernel averages of such runs into the JSON. Nothing here is a pass
mark: both sides of the comparison are this project's code.
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

GRID = 3.0 / 8
CASES = {"cloud_100k": 100000, "cloud_1m": 1000000,
         "rgbd_640x480": (640, 480), "rgbd_1280x720": (1280, 720)}
KERNELS = ("TouchKernel", "ValidKernel", "ParameterizeKernel",
           "DeformCheckKernel", "DeformKernel", "DeformImagePackKernel",
           "ProjectPackKernel", "ResolveKernel", "UnprojectKernel",
           "ToFloatKernel", "TileTotalsKernel", "TileScanKernel")


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e3


def _displaced(slac, points):
    g = slac.ControlGrid(GRID, 1000)
    g.touch(points)
    g.compactify()
    init = g.get_init_positions()
    g.get_curr_positions().copy_(init + 0.02 * torch.sin(init))
    return g


def run_cloud(n, reps):
    from open3d_amd import slac
    gen = torch.Generator(device="cuda").manual_seed(1)
    pts = (torch.rand((n, 3), generator=gen, device="cuda") - 0.5) * 3.0
    nm = torch.nn.functional.normalize(
        torch.randn((n, 3), generator=gen, device="cuda"), dim=1)
    g = _displaced(slac, pts)
    cloud = g.parameterize(pts, nm)
    assert cloud.positions.shape[0] == n
    return {"points": n, "nodes": g.size(),
            "touch_us": _timed(lambda: g.touch(pts), reps),
            "parameterize_us": _timed(lambda: g.parameterize(pts, nm), reps),
            "deform_us": _timed(lambda: g.deform(cloud), reps)}


def run_rgbd(size, reps):
    from open3d_amd import slac, synthetic as syn
    w, h = size
    depth, color, K, Ts = syn.render_frames(0, 1, w, h, device="cuda")
    depth, color, T = depth[0].contiguous(), color[0].contiguous(), Ts[0]
    pts, _ = slac.create_from_rgbd_image(depth, None, K, T)
    g = _displaced(slac, pts)
    fused = g.deform((depth, color), K, T)
    chain = g.deform_seam_by_seam(depth, color, K, T)
    assert torch.equal(fused[0], chain[0]) and torch.equal(fused[1], chain[1])
    return {"width": w, "height": h, "nodes": g.size(),
            "valid_pixels": int(pts.shape[0]),
            "fused_us": _timed(lambda: g.deform((depth, color), K, T), reps),
            "seam_by_seam_us": _timed(
                lambda: g.deform_seam_by_seam(depth, color, K, T), reps)}


def run_case(name, reps):
    spec = CASES[name]
    return run_cloud(spec, reps) if isinstance(spec, int) else \
        run_rgbd(spec, reps)


def kernel_averages(path):
    """Average duration (us) and launches per kernel of a kernel-trace CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            short = next((k for k in KERNELS if k in name), None)
            if short is None:
                continue
            if short == "ResolveKernel":
                short += "<u8>" if "unsigned char" in name else "<f32>"
            ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            out.setdefault(short, []).append(ns)
    return {k: {"launches": len(v), "avg_us": round(sum(v) / len(v) / 1e3, 2),
                "min_us": round(min(v) / 1e3, 2)} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--kernel-trace", nargs="*", default=[],
                    metavar="CASE=CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "control_grid_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        result = json.load(open(a.out))
        for item in a.kernel_trace:
            case, path = item.split("=", 1)
            result["cases"][case]["kernels"] = kernel_averages(path)
        json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
        return 0
    assert torch.cuda.is_available(), "bench_control_grid needs the GPU"
    if a.case:
        print(json.dumps({a.case: run_case(a.case, a.reps)}))
        return 0
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
              "grid_size": GRID,
              "cases": {c: run_case(c, a.reps) for c in CASES}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
