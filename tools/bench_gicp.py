"""Generalized ICP timings on the MI355X.

    python tools/bench_gicp.py [--reps 20] [--out profiles/gicp_bench.json]
                               [--no-kernel-trace]

Records (nothing here is a pass mark; both sides of every comparison are this
project's code):

  accumulate_100k / accumulate_1m
        o3dmi_icp_generalized_accumulate alone on 100 k and 1 M matched pairs,
        Float32, event time of the whole call (the accumulate launch, the
        checked final pass and the wait for the range check's verdict), beside
        o3dmi_icp_p2plane_accumulate on the same pairs, and the bytes of
        DESIGN.md's model (104 B per pair at Float32: 8 B of correspondence
        index, 24 B for the two positions, 72 B for the two covariances) over
        that time.
  icp_generalized / icp_point_to_plane
        one single-scale ICP call, 2 x 100 k points of the synthetic room
        pair, covariances given, and the same call with point-to-plane on the
        same clouds, and their ratio.
  kernels
        average time of GeneralizedAccumulateKernel<float> and
        P2PlaneAccumulateKernel<float> at both sizes, from a kernel-trace run
        of its own: a fresh child process of this file under rocprofv3.
"""
import argparse
import ctypes as C
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL_BYTES_PER_PAIR = 104
SIZES = (100000, 1000000)


def _event_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return float(np.median(us))


def _wall_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t) * 1e6)
    return float(np.median(us))


def _accumulate_calls(n):
    """-> (generalized, p2plane) callables on the same n matched pairs."""
    from open3d_amd import _lib, registration as reg
    from open3d_amd.core import stream
    gen = torch.Generator(device="cuda").manual_seed(7)

    def rnd(*shape):
        return torch.rand(shape, generator=gen, device="cuda") * 2 - 1
    tgt = rnd(n, 3) * 3
    tn = torch.nn.functional.normalize(rnd(n, 3), dim=1)
    corr = torch.randperm(n, generator=gen, device="cuda")
    src = tgt[corr] + 0.02 * rnd(n, 3)
    sn = torch.nn.functional.normalize(tn[corr] + 0.1 * rnd(n, 3), dim=1)
    cs = reg.covariances_from_normals(sn, 1e-3)
    ct = reg.covariances_from_normals(tn, 1e-3)
    sums = torch.zeros(32, dtype=torch.float64, device="cuda")
    R = np.ascontiguousarray(
        [[0.96, -0.28, 0.0], [0.28, 0.96, 0.0], [0.0, 0.0, 1.0]])
    L = _lib.lib()

    def generalized():
        _lib.check(L.o3dmi_icp_generalized_accumulate(
            _lib.ptr(src), _lib.ptr(cs), _lib.ptr(tgt), _lib.ptr(ct),
            _lib.ptr(corr), n, n, _lib.F32, _lib.f64p(R), 0, C.c_double(1.0),
            C.c_double(1.0), _lib.ptr(sums), stream()),
            "generalized_accumulate")

    def p2plane():
        _lib.check(L.o3dmi_icp_p2plane_accumulate(
            _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(tn), _lib.ptr(corr), n,
            _lib.F32, 0, C.c_double(1.0), C.c_double(1.0), _lib.ptr(sums),
            stream()), "p2plane_accumulate")
    return generalized, p2plane, sums


def run_accumulate(n, reps):
    generalized, p2plane, sums = _accumulate_calls(n)
    us = _event_us(generalized, reps)
    assert float(sums[28]) == n and float(sums[29]) == 0
    us_plane = _event_us(p2plane, reps)
    return {"pairs": n, "call_us": us, "p2plane_call_us": us_plane,
            "ratio_over_p2plane": us / us_plane,
            "model_GBps": n * MODEL_BYTES_PER_PAIR / us * 1e-3}


def run_icp(reps):
    from open3d_amd import registration as reg, synthetic as syn
    n = 100000
    p = syn.make_icp_pair(n, n, seed=0)
    src, tgt, nrm = (torch.from_numpy(np.ascontiguousarray(a)).cuda()
                     for a in (p["source"], p["target"], p["target_normals"]))
    sn = reg.estimate_normals(src, max_nn=20)
    cs = reg.covariances_from_normals(sn, 1e-3)
    ct = reg.covariances_from_normals(nrm, 1e-3)
    crit = reg.ICPConvergenceCriteria(1e-6, 1e-6, 30)
    out = {}

    def generalized():
        out["generalized"] = reg.icp(
            src, tgt, None, 0.07, criteria=crit,
            estimation_method=reg.TransformationEstimationForGeneralizedICP(),
            source_covariances=cs, target_covariances=ct)

    def plane():
        out["plane"] = reg.icp(src, tgt, nrm, 0.07, criteria=crit)
    res = {"points": n,
           "icp_generalized_us": _wall_us(generalized, reps),
           "icp_point_to_plane_us": _wall_us(plane, reps)}
    for k in ("generalized", "plane"):
        res[k + "_iterations"] = out[k].num_iterations
        res[k + "_fitness"] = out[k].fitness
    res["ratio_generalized_over_point_to_plane"] = (
        res["icp_generalized_us"] / res["icp_point_to_plane_us"])
    res["per_iteration_ratio"] = (
        res["icp_generalized_us"] / max(out["generalized"].num_iterations, 1)
    ) / (res["icp_point_to_plane_us"] / max(out["plane"].num_iterations, 1))
    return res


def traced_child():
    """The body of the kernel-trace run: five calls of each seam per size."""
    for n in SIZES:
        generalized, p2plane, _ = _accumulate_calls(n)
        for _ in range(5):
            generalized()
            p2plane()
        torch.cuda.synchronize()


def run_kernel_trace():
    """-> {kernel name: {pairs: average us}} from a child under rocprofv3."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "-d", d, "-o", "gicp", "--",
               sys.executable, os.path.abspath(__file__), "--traced-child"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return {"error": (r.stderr or r.stdout)[-400:]}
        rows = sqlite3.connect(dbs[0]).execute(
            "select name, end - start from kernels order by start").fetchall()
    out = {}
    for key in ("GeneralizedAccumulateKernel", "P2PlaneAccumulateKernel"):
        t = [dt for name, dt in rows if key in name]
        # launches alternate per size: the first five of each kernel are the
        # 100 k pairs, the last five the 1 M
        if len(t) == 10:
            out[key] = {str(SIZES[0]): float(np.mean(t[:5])) / 1e3,
                        str(SIZES[1]): float(np.mean(t[5:])) / 1e3}
        else:
            out[key] = {"launches": len(t)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "gicp_bench.json"))
    ap.add_argument("--no-kernel-trace", action="store_true")
    ap.add_argument("--traced-child", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gicp needs the GPU"
    if a.traced_child:
        traced_child()
        return 0
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
              "note": "recorded, not a pass mark",
              "accumulate_100k": run_accumulate(SIZES[0], a.reps),
              "accumulate_1m": run_accumulate(SIZES[1], a.reps),
              "icp": run_icp(a.reps)}
    if not a.no_kernel_trace:
        result["kernels_us"] = run_kernel_trace()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
