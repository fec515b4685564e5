"""Rigid multiway fragment optimisation on one MI355X ->
profiles/slac_rigid_bench.json.

    python tools/bench_slac.py [--out profiles/slac_rigid_bench.json]

(a) One iteration's fill for E = 8 and 32 edges of about 50 k and 200 k
    correspondences (8 fragments of 200 k points, random matched rows: the
    gathers have no locality), Float32, warm, median of 5, device-synchronised:
    o3dmi_slac_rigid_terms (one launch for all edges, table upload and the
    host wait included) against E calls of the seam form
    o3dmi_fill_in_rigid_alignment_term, each preceded by the three row gathers
    and the three transforms a dispatcher issues for it.
(b) The whole optimizer at upstream's defaults on the scene of
    tests/_slac_oracle.make_scene.
(c) The numpy restatement's time on the same input ("restated CPU path") and
    its order sensitivity d (the pose tolerance of tests/test_slac_gpu.py).

Kernel times come from runs of their own under the kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/fill_E_C -o t \\
        -- python tools/bench_slac.py --leg fill --edges E --count C \\
        > DIR/fill_E_C.json
    rocprofv3 ... -d DIR/operator -o t -- python tools/bench_slac.py \\
        --leg operator > DIR/operator.json
    python tools/bench_slac.py --merge DIR

fill: RigidTermsKernel alone, against the 52 B / correspondence model (16 B of
indices + 36 B of gathered rows); operator: launches per iteration.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from open3d_amd import _lib, slac  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

MODEL_BYTES = 52
FILL_CASES = [(8, 50000), (8, 200000), (32, 50000), (32, 200000)]
THRESHOLD = 0.07


def timed(fn, repeat=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms


def fill_setup(n_edges, count, n_frag=8, n_pts=200000, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    base = torch.rand((n_pts, 3), generator=g) * 2 - 1
    nrm = torch.nn.functional.normalize(torch.randn((n_pts, 3), generator=g))
    frags, inv = [], []
    for _ in range(n_frag):
        perm = torch.randperm(n_pts, generator=g)
        p = base + 0.01 * torch.randn((n_pts, 3), generator=g)
        frags.append((p[perm].contiguous().cuda(),
                      nrm[perm].contiguous().cuda()))
        iv = torch.empty_like(perm)
        iv[perm] = torch.arange(n_pts)
        inv.append(iv)
    poses = [np.eye(4) for _ in range(n_frag)]
    for k, T in enumerate(poses):
        T[:3, 3] = 0.002 * k
    edges, sets = [], []
    for e in range(n_edges):
        i, j = e % n_frag, (e + 1 + e // n_frag) % n_frag
        m = torch.randint(0, n_pts, (count,), generator=g)
        edges.append((i, j))
        sets.append(torch.stack([inv[i][m], inv[j][m]], 1).contiguous().cuda())
    return frags, poses, edges, sets


def batched_fill(frags, poses, edges, sets):
    out = torch.zeros((len(edges), 29), dtype=torch.float64, device="cuda")

    def run():
        slac.rigid_terms(frags, poses, edges, sets, THRESHOLD, out=out)
    return run, out


def seam_fill(frags, poses, edges, sets):
    L = _lib.lib()
    n = 6 * len(frags)
    AtA = torch.zeros((n, n), device="cuda")
    Atb = torch.zeros(n, device="cuda")
    res = torch.zeros(1, device="cuda")

    def run():
        AtA.zero_()
        Atb.zero_()
        res.zero_()
        for (i, j), cs in zip(edges, sets):
            a, b = cs[:, 0], cs[:, 1]
            p = frags[i][0].index_select(0, a)
            nn = frags[i][1].index_select(0, a)
            q = frags[j][0].index_select(0, b)
            Ti = np.ascontiguousarray(poses[i])
            Tj = np.ascontiguousarray(poses[j])
            _lib.check(L.o3dmi_transform_points(
                _lib.f64p(Ti), _lib.ptr(p), p.shape[0], _lib.F32, stream()),
                "transform")
            _lib.check(L.o3dmi_transform_normals(
                _lib.f64p(Ti), _lib.ptr(nn), p.shape[0], _lib.F32, stream()),
                "transform")
            _lib.check(L.o3dmi_transform_points(
                _lib.f64p(Tj), _lib.ptr(q), p.shape[0], _lib.F32, stream()),
                "transform")
            slac.fill_in_rigid_alignment_term(AtA, Atb, res, p, q, nn, i, j,
                                              THRESHOLD)
    return run


def fill_case(n_edges, count):
    frags, poses, edges, sets = fill_setup(n_edges, count)
    run_b, out = batched_fill(frags, poses, edges, sets)
    ms_b, runs_b = timed(run_b)
    ms_s, runs_s = timed(seam_fill(frags, poses, edges, sets))
    pairs = n_edges * count
    return dict(edges=n_edges, correspondences_per_edge=count,
                pairs_within_threshold=int(out[:, 28].sum().item()),
                batched_wall_ms=ms_b, batched_runs_ms=runs_b,
                seam_calls_wall_ms=ms_s, seam_runs_ms=runs_s,
                seam_over_batched=ms_s / ms_b,
                batched_wall_model_GBps=pairs * MODEL_BYTES / (ms_b * 1e6))


def scene_graph():
    import _slac_oracle as so
    frags, truth, start, edges = so.make_scene()
    g = [(torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda())
         for p, n in frags]
    return so, frags, truth, start, edges, g


def operator_case():
    so, frags, truth, start, edges, g = scene_graph()
    graph = slac.PoseGraph(start, edges)
    params = slac.SLACOptimizerParams()
    info = {}

    def run():
        info["r"] = slac.run_rigid_optimizer_for_fragments(
            g, graph, params, return_info=True)
    ms, runs = timed(run, 3)
    zero = slac.SLACOptimizerParams(max_iterations=0)
    ms0, _ = timed(lambda: slac.run_rigid_optimizer_for_fragments(
        g, graph, zero), 3)
    t0 = time.perf_counter()
    want = so.rigid_optimize(frags, start, edges)
    oracle_s = time.perf_counter() - t0
    rev = so.rigid_optimize(frags, start, edges, reverse=True)
    d = max(float(np.abs(a - b).max())
            for a, b in zip(want["poses"], rev["poses"]))
    got, ginfo = info["r"]
    worst = max(float(np.abs(a - b).max())
                for a, b in zip(got.nodes, want["poses"]))
    return dict(
        nodes=len(frags), edges=len(edges),
        points_per_fragment=[int(f[0].shape[0]) for f in frags],
        correspondences=[int(c) for c in ginfo["n_corres"]],
        iterations=params.max_iterations,
        wall_ms=ms, runs_ms=runs, correspondence_sets_wall_ms=ms0,
        per_iteration_ms=(ms - ms0) / params.max_iterations,
        host_waits_per_iteration=1,
        losses=[float(v) for v in ginfo["losses"]],
        restated_cpu_path_s=oracle_s,
        oracle_order_sensitivity_d=d,
        worst_pose_entry_difference_to_oracle=worst,
        relative_pose_errors_before=so.relative_errors(start, truth),
        relative_pose_errors_after=so.relative_errors(got.nodes, truth))


def leg(name, n_edges, count):
    """One leg for a kernel-trace run of its own; prints one JSON line."""
    if name == "fill":
        frags, poses, edges, sets = fill_setup(n_edges, count)
        run, _ = batched_fill(frags, poses, edges, sets)
        ms, runs = timed(run)
        print(json.dumps(dict(leg=name, edges=n_edges, count=count, calls=6,
                              wall_ms=ms, runs_ms=runs)))
        return
    _, _, _, start, edges, g = scene_graph()
    graph = slac.PoseGraph(start, edges)
    params = slac.SLACOptimizerParams()
    ms, runs = timed(lambda: slac.run_rigid_optimizer_for_fragments(
        g, graph, params), 3)
    print(json.dumps(dict(leg=name, calls=4, iterations=params.max_iterations,
                          edges=len(edges), wall_ms=ms, runs_ms=runs)))


def kernel_rows(d):
    """(name, duration ns) of every launch in a rocprofv3 csv kernel trace."""
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
    for (n_edges, count) in FILL_CASES:
        sub = os.path.join(d, "fill_%d_%d" % (n_edges, count))
        rows = kernel_rows(sub)
        ks = [ns for k, ns in rows if "RigidTermsKernel" in k]
        fin = [ns for k, ns in rows if "RigidTermsFinalKernel" in k]
        ks = ks[1:] or ks                      # first launch: warm-up
        us = float(np.median(ks)) / 1e3
        pairs = n_edges * count
        trace["%d_x_%d" % (n_edges, count)] = dict(
            launches=len(ks) + 1, rigid_terms_kernel_us_median=us,
            final_pass_us_median=float(np.median(fin)) / 1e3,
            correspondences_per_s=pairs / (us * 1e-6),
            model_bytes_per_correspondence=MODEL_BYTES,
            model_GBps=pairs * MODEL_BYTES / (us * 1e3))
    sub = os.path.join(d, "operator")
    with open(sub + ".json") as f:
        info = json.loads(f.read().strip().splitlines()[-1])
    rows = kernel_rows(sub)
    terms = [ns for k, ns in rows if "RigidTermsKernel" in k]
    trace["operator"] = dict(
        launches_per_call=len(rows) / info["calls"],
        rigid_terms_launches_per_iteration=len(terms) /
        (info["calls"] * info["iterations"]),
        launches_per_iteration=2,
        rigid_terms_kernel_us_median=float(np.median(terms)) / 1e3,
        kernel_ms_per_call=sum(ns for _, ns in rows) / info["calls"] / 1e6,
        wall_ms_under_trace=info["wall_ms"])
    res["kernel_trace"] = trace
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(trace))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "slac_rigid_bench.json"))
    ap.add_argument("--leg", choices=["fill", "operator"])
    ap.add_argument("--edges", type=int, default=8)
    ap.add_argument("--count", type=int, default=50000)
    ap.add_argument("--merge", help="directory of the per-leg trace runs")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.edges, a.count)
    if a.merge:
        return merge(a.merge, a.out)
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32",
               fill=[fill_case(e, c) for e, c in FILL_CASES],
               operator=operator_case())
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
