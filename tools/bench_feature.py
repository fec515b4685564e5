"""FPFH and feature-correspondence timings on the MI355X.

    python tools/bench_feature.py [--reps 5] [--out profiles/feature_bench.json]

FPFH: a voxel-down-sampled synthetic surface (the bumpy sphere of
tests/test_feature_gpu.py, scaled to ~100 k and ~1 M points), hybrid search
with radius = 5 voxels and max_nn = 100. Correspondences: uniform random
33-D features, N = M = 10 k and 50 k, with and without the mutual filter.
Times are device events around whole operator calls (median of --reps after
one warm-up). FLOP come from shapes: 2 N M 33 useful, against the 157.3 TF
float32 matrix peak; and the kernel's own float64 operations (sub, mul, add
per element, K padded to whole chunks), against the float64 VALU's issue
rate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 157.3e12
F64_VECTOR_OPS = 39.3e12  # 78.6 TF counts an FMA as two; sub, mul, add are one each
NN_KC = 12  # csrc/feature.hip kNnKc


def surface(n, seed=0):
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th = np.arctan2(v[:, 1], v[:, 0])
    ph = np.arccos(np.clip(v[:, 2], -1, 1))
    r = 1.0 + 0.08 * np.sin(5 * th) * np.sin(4 * ph) + 0.05 * np.cos(7 * ph)
    return (v * r[:, None]).astype(np.float32)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [float(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["fpfh", "corr"], default=None,
                    help="one half only (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "feature_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_feature needs the GPU"
    from open3d_amd import registration as reg
    res = {"fpfh": [], "correspondences": []}
    fpfh_sizes = [] if a.only == "corr" else [(100_000, 400_000),
                                              (1_000_000, 4_000_000)]
    for target, raw in fpfh_sizes:
        pts = torch.from_numpy(surface(raw)).cuda()
        area = 4 * np.pi * 1.05 ** 2
        voxel = float(np.sqrt(area / target))
        p, _ = reg.voxel_down_sample(pts, None, voxel)
        n = reg.estimate_normals(p, max_nn=30)
        ms, all_ms = timed(lambda: reg.compute_fpfh_feature(
            p, n, max_nn=100, radius=5 * voxel), a.reps)
        res["fpfh"].append(dict(points=int(p.shape[0]), voxel=voxel,
                                radius=5 * voxel, max_nn=100, ms=ms,
                                all_ms=all_ms))
        print("fpfh", res["fpfh"][-1], flush=True)
    rng = np.random.RandomState(1)
    for N in ((10_000, 50_000) if a.only != "fpfh" else ()):
        s = torch.from_numpy(rng.uniform(0, 1, (N, 33)).astype(np.float32))
        t = torch.from_numpy(rng.uniform(0, 1, (N, 33)).astype(np.float32))
        s, t = s.cuda(), t.cuda()
        for mutual in (False, True):
            ms, all_ms = timed(lambda: reg.correspondences_from_features(
                s, t, mutual_filter=mutual), a.reps)
            sweeps = 2 if mutual else 1
            useful = 2.0 * N * N * 33 * sweeps
            padded = 3.0 * N * N * (-(-33 // NN_KC) * NN_KC) * sweeps
            res["correspondences"].append(dict(
                n=N, m=N, dim=33, mutual_filter=mutual, ms=ms, all_ms=all_ms,
                useful_flop=useful,
                kernel_f64_ops=padded,
                share_f32_matrix_peak=useful / (ms * 1e-3) / F32_MATRIX_PEAK,
                share_f64_vector_issue=padded / (ms * 1e-3) / F64_VECTOR_OPS))
            print("corr", res["correspondences"][-1], flush=True)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"fpfh_ms": [r["ms"] for r in res["fpfh"]],
                      "corr_ms": [r["ms"] for r in res["correspondences"]]}))


if __name__ == "__main__":
    main()
