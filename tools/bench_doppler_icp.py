"""Doppler ICP timings on the MI355X.

    python tools/bench_doppler_icp.py [--reps 20] [--out profiles/doppler_icp_bench.json]

Records (nothing here is a pass mark; both sides of every comparison are this
project's code):

  accumulate_100k / accumulate_1m
        o3dmi_icp_doppler_accumulate alone on 100 k and 1 M matched pairs,
        Float32, event time of the whole call (the accumulate launch, the
        checked final pass and the wait for the range check's verdict), and
        the bytes of DESIGN.md's model (60 B per pair) over that time.
  icp_doppler / icp_point_to_plane
        one single-scale ICP call, 2 x 100 k points of the synthetic room pair
        with synthetic dopplers (the estimator's own prediction at the true
        motion), and the same call with point-to-plane on the same clouds --
        the yardstick, because that is the code the library had before on
        identical input -- and their ratio.
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

MODEL_BYTES_PER_PAIR = 60


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


def run_accumulate(n, reps):
    from open3d_amd import _lib
    from open3d_amd.core import stream
    gen = torch.Generator(device="cuda").manual_seed(7)

    def rnd(*shape):
        return torch.rand(shape, generator=gen, device="cuda") * 2 - 1
    tgt = rnd(n, 3) * 3
    tn = torch.nn.functional.normalize(rnd(n, 3), dim=1)
    corr = torch.randperm(n, generator=gen, device="cuda")
    src = tgt[corr] + 0.02 * rnd(n, 3)
    dirs = torch.nn.functional.normalize(src, dim=1)
    dops = rnd(n)
    sums = torch.zeros(29, dtype=torch.float64, device="cuda")
    f64 = C.POINTER(C.c_double)
    R = np.eye(3).reshape(9)
    r = np.array([0.4, -0.2, 0.3])
    w = np.array([0.1, -0.2, 0.3])
    v = np.array([0.5, 0.2, -0.1])
    L = _lib.lib()

    def call():
        _lib.check(L.o3dmi_icp_doppler_accumulate(
            _lib.ptr(src), _lib.ptr(dops), _lib.ptr(dirs), _lib.ptr(tgt),
            _lib.ptr(tn), _lib.ptr(corr), n, n, _lib.F32,
            R.ctypes.data_as(f64), r.ctypes.data_as(f64),
            w.ctypes.data_as(f64), v.ctypes.data_as(f64), C.c_double(0.1), 0,
            C.c_double(2.0), 0, C.c_double(1.0), C.c_double(1.0), 0,
            C.c_double(1.0), C.c_double(1.0), C.c_double(0.01),
            _lib.ptr(sums), stream()), "doppler_accumulate")
    us = _event_us(call, reps)
    assert float(sums[28]) == n
    return {"pairs": n, "call_us": us,
            "model_GBps": n * MODEL_BYTES_PER_PAIR / us * 1e-3}


def run_icp(reps):
    from open3d_amd import registration as reg, synthetic as syn
    n = 100000
    p = syn.make_icp_pair(n, n, seed=0)
    dirs = reg.compute_direction_vectors(p["source"])
    # -d . v with v = -t / period: the estimator's prediction for a pure
    # translation; the rotation's share comes out as residual
    period = 0.1
    dops = (dirs @ (p["T_gt"][:3, 3] / period)).astype(np.float32)
    src, tgt, nrm, dd, dr = (torch.from_numpy(np.ascontiguousarray(a)).cuda()
                             for a in (p["source"], p["target"],
                                       p["target_normals"], dops,
                                       dirs.astype(np.float32)))
    crit = reg.ICPConvergenceCriteria(1e-6, 1e-6, 30)
    out = {}

    def doppler():
        out["doppler"] = reg.icp(
            src, tgt, nrm, 0.07, criteria=crit,
            estimation_method=reg.TransformationEstimationForDopplerICP(),
            source_dopplers=dd, source_directions=dr)

    def plane():
        out["plane"] = reg.icp(src, tgt, nrm, 0.07, criteria=crit)
    res = {"points": n,
           "icp_doppler_us": _wall_us(doppler, reps),
           "icp_point_to_plane_us": _wall_us(plane, reps)}
    for k in ("doppler", "plane"):
        res[k + "_iterations"] = out[k].num_iterations
        res[k + "_fitness"] = out[k].fitness
    res["ratio_doppler_over_point_to_plane"] = (
        res["icp_doppler_us"] / res["icp_point_to_plane_us"])
    res["per_iteration_ratio"] = (
        res["icp_doppler_us"] / max(out["doppler"].num_iterations, 1)) / (
        res["icp_point_to_plane_us"] / max(out["plane"].num_iterations, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "doppler_icp_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_doppler_icp needs the GPU"
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
              "note": "recorded, not a pass mark",
              "accumulate_100k": run_accumulate(100000, a.reps),
              "accumulate_1m": run_accumulate(1000000, a.reps),
              "icp": run_icp(a.reps)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
