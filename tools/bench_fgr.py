"""Fast Global Registration on one MI355X -> profiles/fgr_bench.json.

    python tools/bench_fgr.py [--out profiles/fgr_bench.json]

Two samplings of a synthetic room (floor, two walls, eight objects), the second
moved, both voxel-down-sampled at 1 cm (asked for 5 k and 20 k points, the
grid leaves about 9 k and 37 k), Float32,
with normals and FPFH (max_nn 100, radius 5 voxels). Warm, median of 10
event-timed calls, host waits included:
  * whole: registration_fgr_based_on_feature_matching at upstream's defaults;
  * ransac: registration_ransac_based_on_feature_matching on the same pair
    (mutual filter, edge length 0.9 + distance 1.5 voxels, 100 000 / 0.999);
  * optimize: o3dmi_fgr_optimize alone on 3000 correspondences (half of them
    random), 64 iterations, in the resident and in the streamed form;
  * upstream_shape: a restatement of upstream's shape on this library: per
    iteration one streamed step (gather, sums, finish launches), a download
    of delta, trans composed on the host, delta uploaded again and q moved
    by a launch of its own: 64 host hops.
Both sides of every comparison are this project's code: recorded, not a pass
mark. Kernel times come from runs of their own under the kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/LEG -o t -- \
        python tools/bench_fgr.py --leg LEG > DIR/LEG.json
    python tools/bench_fgr.py --merge DIR    # LEG in resident, streamed, whole
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open3d_amd import _lib, registration as reg  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

VOXEL = 0.01
RESIDENT, STREAMED = 1, 2


def room(n_target, seed):
    rng = np.random.RandomState(seed)
    side = np.sqrt(n_target * VOXEL * VOXEL / 2.6)
    dense = int(n_target * 6)
    k = dense // 2
    parts = [np.column_stack([rng.uniform(0, side, (k, 2)), np.zeros(k)])]
    k = dense // 6
    h = 0.6 * side
    parts.append(np.column_stack([rng.uniform(0, side, k), np.zeros(k),
                                  rng.uniform(0, h, k)]))
    parts.append(np.column_stack([np.zeros(k), rng.uniform(0, side, k),
                                  rng.uniform(0, h, k)]))
    k = dense // 48
    shapes = np.random.RandomState(7)  # the same objects in both samplings
    for j in range(8):
        c = np.array([(0.15 + 0.2 * (j % 4) + 0.05 * shapes.uniform()) * side,
                      (0.25 + 0.4 * (j // 4) + 0.1 * shapes.uniform()) * side,
                      (0.1 + 0.2 * shapes.uniform()) * side])
        r = (0.04 + 0.04 * shapes.uniform()) * side
        if j % 2:
            v = rng.normal(size=(k, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
        else:
            v = rng.uniform(-1, 1, (k, 3))
            face = rng.randint(0, 3, k)
            v[np.arange(k), face] = np.sign(v[np.arange(k), face])
        parts.append(c + r * v)
    pts = np.vstack(parts)
    pts += rng.normal(scale=VOXEL / 10, size=pts.shape)
    return pts


def motion():
    a = 0.6
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0],
                 [0, 0, 1]]
    T[:3, 3] = [0.2, -0.1, 0.05]
    return T


def pair(n_target):
    T = motion()
    a = room(n_target, 1).astype(np.float32)
    b = (room(n_target, 2) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    out = []
    for pts in (a, b):
        p, _ = reg.voxel_down_sample(torch.from_numpy(pts).cuda(), None, VOXEL)
        p = p.contiguous()
        nrm = reg.estimate_normals(p, 30, 3 * VOXEL)
        f = reg.compute_fpfh_feature(p, nrm, 100, 5 * VOXEL)
        out += [p, nrm, f]
    return out + [T]


def _once(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    ms = sorted(_once(fn) for _ in range(reps))
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def rotation_error(T, T_true):
    R = T[:3, :3].T @ T_true[:3, :3]
    f = np.linalg.norm(R - np.eye(3))
    return float(2 * np.arcsin(min(1.0, f / (2 * np.sqrt(2)))))


def whole_case(n_target):
    S, Sn, Fs, Tg, Tn, Ft, T = pair(n_target)
    last = {}

    def fgr():
        last["fgr"] = reg.registration_fgr_based_on_feature_matching(
            S, Tg, Fs, Ft, reg.FastGlobalRegistrationOption())
    out = dict(source_points=int(S.shape[0]), target_points=int(Tg.shape[0]))
    out["fgr"] = timed(fgr)
    res, info = last["fgr"]
    out["fgr"].update(info=info, fitness=res.fitness,
                      inlier_rmse=res.inlier_rmse,
                      rotation_error_rad=rotation_error(res.transformation, T))
    checkers = [reg.CorrespondenceCheckerBasedOnEdgeLength(0.9),
                reg.CorrespondenceCheckerBasedOnDistance(1.5 * VOXEL)]

    def ransac():
        last["ransac"] = reg.registration_ransac_based_on_feature_matching(
            S, Tg, Fs, Ft, True, 1.5 * VOXEL, None, 3, checkers,
            reg.RANSACConvergenceCriteria(100000, 0.999), seed=0)
    out["ransac"] = timed(ransac)
    g = last["ransac"]
    out["ransac"].update(iterations_run=int(g.iterations_run),
                         rounds=int(g.num_batches), fitness=g.fitness,
                         inlier_rmse=g.inlier_rmse,
                         rotation_error_rad=rotation_error(g.transformation,
                                                           T))
    return out


def optimize_inputs(n_corres=3000, n=5000, seed=3):
    """Two normalised float64 clouds and n_corres pairs, half of them random."""
    rng = np.random.RandomState(seed)
    T = motion()
    src = rng.uniform(-0.5, 0.5, (n, 3)) * [2.0, 1.4, 0.8]
    tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.002, (n, 3))
    src = src - src.mean(0)
    tgt = tgt - tgt.mean(0)
    scale = max(np.linalg.norm(src, axis=1).max(),
                np.linalg.norm(tgt, axis=1).max())
    rows = rng.randint(0, n, n_corres)
    bad = rng.uniform(size=n_corres) < 0.5
    cols = np.where(bad, rng.randint(0, n, n_corres), rows)
    return (torch.from_numpy(src / scale).cuda(),
            torch.from_numpy(tgt / scale).cuda(),
            torch.from_numpy(np.stack([rows, cols], 1).astype(np.int64)).cuda(),
            1.0)


def optimizer(S, Tg, Cg, par, form, iterations=64):
    L = _lib.lib()
    n = Cg.shape[0]
    out = torch.zeros(18, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(L.o3dmi_internal_fgr_stream_scratch_bytes(n) // 8 + 1,
                          dtype=torch.float64, device="cuda")

    def run():
        _lib.check(L.o3dmi_internal_fgr_optimize(
            _lib.ptr(S), S.shape[0], _lib.ptr(Tg), Tg.shape[0], _lib.ptr(Cg),
            n, C.c_double(par), C.c_double(1.4), 1, C.c_double(0.025),
            iterations, form, _lib.ptr(scratch), _lib.ptr(out), None,
            stream()), "fgr_optimize")
    return run, out


def upstream_shape(S, Tg, Cg, par):
    """64 x (one streamed step, download, host compose, upload, move)."""
    L = _lib.lib()
    q = Tg.clone()
    out = torch.zeros(18, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(
        L.o3dmi_internal_fgr_stream_scratch_bytes(Cg.shape[0]) // 8 + 1,
        dtype=torch.float64, device="cuda")
    state = {}

    def run():
        q.copy_(Tg)
        trans = np.eye(4)
        p = par
        for itr in range(64):
            _lib.check(L.o3dmi_internal_fgr_optimize(
                _lib.ptr(S), S.shape[0], _lib.ptr(q), q.shape[0],
                _lib.ptr(Cg), Cg.shape[0], C.c_double(p), C.c_double(1.4), 0,
                C.c_double(0.025), 1, STREAMED, _lib.ptr(scratch),
                _lib.ptr(out), None, stream()), "fgr_optimize")
            delta = out[:16].cpu().numpy().reshape(4, 4)    # the host hop
            trans = delta @ trans
            d = torch.from_numpy(delta).cuda()              # and back
            q.copy_(q @ d[:3, :3].T + d[:3, 3])
            if itr % 4 == 0 and p > 0.025:
                p /= 1.4
        state["trans"] = trans
    return run, state


def optimize_case():
    S, Tg, Cg, par = optimize_inputs()
    out = dict(correspondences=int(Cg.shape[0]), iterations=64)
    res = {}
    for name, form in (("resident", RESIDENT), ("streamed", STREAMED)):
        run, o = optimizer(S, Tg, Cg, par, form)
        out[name] = timed(run)
        res[name] = o.cpu().numpy().copy()
    out["forms_bit_equal"] = bool(res["resident"].tobytes() ==
                                  res["streamed"].tobytes())
    run, state = upstream_shape(S, Tg, Cg, par)
    out["upstream_shape"] = timed(run)
    d = state["trans"] - res["resident"][:16].reshape(4, 4)
    out["upstream_shape"]["max_abs_difference_to_resident"] = float(
        np.abs(d).max())
    out["streamed_over_resident"] = (out["streamed"]["median_ms"] /
                                     out["resident"]["median_ms"])
    out["upstream_shape_over_resident"] = (
        out["upstream_shape"]["median_ms"] / out["resident"]["median_ms"])
    return out


def leg(name):
    """One leg for a kernel-trace run of its own; prints one JSON line."""
    calls = 5
    if name == "whole":
        S, Sn, Fs, Tg, Tn, Ft, T = pair(5000)

        def run():
            reg.registration_fgr_based_on_feature_matching(
                S, Tg, Fs, Ft, reg.FastGlobalRegistrationOption())
    else:
        S, Tg, Cg, par = optimize_inputs()
        run, _ = optimizer(S, Tg, Cg, par,
                           RESIDENT if name == "resident" else STREAMED)
    t = timed(run, calls)
    t.update(leg=name, calls=calls + 1)
    print(json.dumps(t))


def kernel_rows(d):
    import csv
    rows = []
    for dp, _, files in os.walk(d):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                with open(os.path.join(dp, f)) as fh:
                    for r in csv.DictReader(fh):
                        rows.append((r["Kernel_Name"],
                                     int(r["End_Timestamp"]) -
                                     int(r["Start_Timestamp"])))
    return rows


def merge(d, out_path):
    with open(out_path) as f:
        res = json.load(f)
    trace = {}
    for name, kernels in (("resident", ("ResidentKernel",)),
                          ("streamed", ("StreamPartialKernel",
                                        "StreamFinishKernel",
                                        "StreamGatherKernel")),
                          ("whole", ("o3dmi",))):
        sub = os.path.join(d, name)
        if not os.path.isdir(sub):
            continue
        with open(sub + ".json") as f:
            info = json.loads(f.read().strip().splitlines()[-1])
        t = dict(calls=info["calls"], wall_ms_under_trace=info["median_ms"])
        rows = kernel_rows(sub)
        for k in kernels:
            ks = [ns for kn, ns in rows if k in kn]
            t[k] = dict(launches_per_call=len(ks) / info["calls"],
                        us_per_call=sum(ks) / 1e3 / info["calls"],
                        us_median=float(np.median(ks)) / 1e3 if ks else 0.0)
        trace[name] = t
    res["kernel_trace"] = trace
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(trace))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "fgr_bench.json"))
    ap.add_argument("--leg", choices=["resident", "streamed", "whole"])
    ap.add_argument("--merge", help="directory of the per-leg trace runs")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg)
    if a.merge:
        return merge(a.merge, a.out)
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32",
               voxel=VOXEL, cases=[whole_case(5000), whole_case(20000)],
               optimize=optimize_case())
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
