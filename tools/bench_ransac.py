"""RANSAC on correspondences on one MI355X -> profiles/ransac_bench.json.

    python tools/bench_ransac.py [--out profiles/ransac_bench.json]

For clouds of about 5 k and 20 k points (two samplings of a bumpy sphere, the
second moved and noisy), Float32, warm, median of 5, device-synchronised:
  * the batched scoring launch for 1024 given transformations against the same
    1024 scored by 1024 calls of o3dmi_registration_evaluate;
  * the whole operator at upstream's defaults (100 000 iterations, confidence
    0.999, edge length 0.9 + distance checkers): wall time, iterations run,
    validations, rounds.
    Twice: on 75 % random correspondences (the bound falls inside the first
    round) and on 92 % (several rounds: what the per-round host hop costs).
Kernel times come from runs of their own under the kernel trace, one per leg:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/LEG_N -o t -- \
        python tools/bench_ransac.py --leg LEG --points N > DIR/LEG_N.json
    python tools/bench_ransac.py --merge DIR   # LEG in score, k1, operator

score / k1: ScoreKernel for 1024 transformations beside HybridSearchK1Kernel
(o3dmi_nns_hybrid_search_k1) on the same 1024 x N queries, the source moved
by each transformation beforehand; operator: launches per call and the share
of the wall time a kernel of the library is running.
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
from open3d_amd import _lib, registration as reg  # noqa: E402
from open3d_amd.core import stream  # noqa: E402


def surface(n, seed):
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th = np.arctan2(v[:, 1], v[:, 0])
    ph = np.arccos(np.clip(v[:, 2], -1, 1))
    r = 1.0 + 0.08 * np.sin(5 * th) * np.sin(4 * ph) + 0.05 * np.cos(7 * ph)
    return v * r[:, None]


def motion():
    a = 0.7
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0],
                 [0, 0, 1]]
    T[:3, 3] = [0.3, -0.2, 0.5]
    return T


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


def setup(n, seed, outliers=0.75):
    """Clouds, correspondences and radius of one case."""
    T = motion()
    src = surface(n, seed)
    tgt = surface(n + n // 20, seed + 1) @ T[:3, :3].T + T[:3, 3]
    tgt += np.random.RandomState(seed + 2).normal(0, 0.003, tgt.shape)
    S = torch.from_numpy(src.astype(np.float32)).cuda()
    Tg = torch.from_numpy(tgt.astype(np.float32)).cuda()
    voxel = float(np.sqrt(4 * np.pi / n))
    r = 1.5 * voxel
    # correspondences: a quarter true nearest pairs, the rest random
    rng = np.random.RandomState(seed + 3)
    rows = rng.randint(0, n, n)
    moved = (S[torch.from_numpy(rows).cuda()].double() @
             torch.from_numpy(T[:3, :3].T).cuda() +
             torch.from_numpy(T[:3, 3]).cuda()).float()
    d = torch.cdist(moved, Tg)
    near = d.argmin(1).cpu().numpy()
    rnd = rng.randint(0, tgt.shape[0], n)
    corres = np.stack([rows, np.where(rng.uniform(size=n) < outliers, rnd,
                                      near)], 1).astype(np.int64)
    Cg = torch.from_numpy(corres).cuda()
    return S, Tg, Cg, T, r


def hypotheses(S, Tg, Cg, b):
    """b transformations: hypotheses of the sample stream, no checkers."""
    L = _lib.lib()
    n = S.shape[0]
    smp = torch.empty((b, 3), dtype=torch.int64, device="cuda")
    Ts = torch.empty((b, 16), dtype=torch.float64, device="cuda")
    ps = torch.empty((b,), dtype=torch.int32, device="cuda")
    _lib.check(L.o3dmi_ransac_hypotheses(
        C.c_uint64(0), 0, b, _lib.ptr(S), n, _lib.ptr(Tg), Tg.shape[0], None,
        None, _lib.F32, _lib.ptr(Cg), n, 3, 0, None, None, _lib.ptr(smp),
        _lib.ptr(Ts), _lib.ptr(ps), stream()), "hypotheses")
    torch.cuda.synchronize()
    return Ts


def index(Tg, r):
    h = C.c_void_p()
    _lib.check(_lib.lib().o3dmi_nns_create(
        _lib.ptr(Tg), Tg.shape[0], _lib.F32, C.c_double(r), stream(),
        C.byref(h)), "nns_create")
    return h


def batched_scorer(S, Tg, Cg, Ts, h, with_corres=True):
    L = _lib.lib()
    n, b = S.shape[0], Ts.shape[0]
    cnt = torch.empty((b,), dtype=torch.int64, device="cuda")
    cor = torch.empty((b,), dtype=torch.int64, device="cuda")
    d2 = torch.empty((b,), dtype=torch.float64, device="cuda")
    scratch = torch.empty(
        (L.o3dmi_ransac_score_scratch_bytes(n, b) + 7) // 8,
        dtype=torch.float64, device="cuda")

    def run():
        _lib.check(L.o3dmi_ransac_score(
            h, _lib.ptr(S), n, _lib.ptr(Tg), Tg.shape[0], _lib.ptr(Ts), b,
            _lib.ptr(Cg) if with_corres else None, Cg.shape[0],
            _lib.ptr(cnt), _lib.ptr(d2),
            _lib.ptr(cor) if with_corres else None, _lib.ptr(scratch),
            stream()), "score")
    return run


def operator(S, Tg, Cg, T, r):
    checkers = [reg.CorrespondenceCheckerBasedOnEdgeLength(0.9),
                reg.CorrespondenceCheckerBasedOnDistance(r)]
    last = {}

    def whole():
        last["r"] = reg.registration_ransac_based_on_correspondence(
            S, Tg, Cg, r, None, 3, checkers,
            reg.RANSACConvergenceCriteria(100000, 0.999), seed=0)
    ms_w, all_w = timed(whole)
    g = last["r"]
    dR = g.transformation[:3, :3].T @ T[:3, :3]
    return dict(
        wall_ms=ms_w, runs_ms=all_w, iterations_run=int(g.iterations_run),
        final_iteration_bound=int(g.final_iteration_bound),
        validations=int(g.num_validations), rounds=int(g.num_batches),
        best_iteration=int(g.best_iteration), fitness=g.fitness,
        rotation_error_rad=float(np.arccos(np.clip((np.trace(dR) - 1) / 2,
                                                    -1, 1))))


def case(n, seed):
    L = _lib.lib()
    S, Tg, Cg, T, r = setup(n, seed)
    out = dict(points=n, target_points=int(Tg.shape[0]),
               correspondences=n, max_distance=r)
    b = 1024
    Ts = hypotheses(S, Tg, Cg, b)
    h = index(Tg, r)
    ms_b, all_b = timed(batched_scorer(S, Tg, Cg, Ts, h))
    torch.cuda.synchronize()
    L.o3dmi_nns_destroy(h)
    Th = Ts.cpu().numpy()
    res = _lib.RegistrationResultC()

    def one_by_one():
        for k in range(b):
            _lib.check(L.o3dmi_registration_evaluate(
                _lib.ptr(S), n, _lib.ptr(Tg), Tg.shape[0], _lib.F32,
                C.c_double(r), _lib.f64p(Th[k]), None, C.byref(res),
                stream()), "evaluate")
    ms_e, all_e = timed(one_by_one)
    out["score_1024"] = dict(
        batched_ms=ms_b, runs_ms=all_b, evaluate_calls_ms=ms_e,
        evaluate_runs_ms=all_e, ratio=ms_e / ms_b,
        nn_queries_per_s=b * n / (ms_b * 1e-3))

    out["operator_defaults"] = operator(S, Tg, Cg, T, r)
    S2, Tg2, Cg2, T2, r2 = setup(n, seed, outliers=0.92)
    out["operator_defaults_92pct_random"] = operator(S2, Tg2, Cg2, T2, r2)
    return out


def leg(name, n):
    """One leg for a kernel-trace run of its own; prints one JSON line."""
    L = _lib.lib()
    seed = 100 if n <= 5000 else 200
    b, calls = 1024, 5
    if name == "operator":
        S, Tg, Cg, T, r = setup(n, seed, outliers=0.92)
        torch.cuda.synchronize()
        res = operator(S, Tg, Cg, T, r)      # 1 warm-up + 5 timed calls
        res.update(leg=name, points=n, calls=6)
        print(json.dumps(res))
        return
    S, Tg, Cg, T, r = setup(n, seed)
    Ts = hypotheses(S, Tg, Cg, b)
    h = index(Tg, r)
    if name == "score":
        run = batched_scorer(S, Tg, Cg, Ts, h, with_corres=False)
    else:
        # the same queries, moved beforehand: {b * n, 3}
        M = Ts.reshape(b, 4, 4).float()
        q = (torch.einsum("bij,nj->bni", M[:, :3, :3], S) +
             M[:, None, :3, 3]).reshape(-1, 3).contiguous()
        idx = torch.empty((b * n,), dtype=torch.int32, device="cuda")
        d2 = torch.empty((b * n,), dtype=torch.float32, device="cuda")
        cnt = torch.empty((b * n,), dtype=torch.int32, device="cuda")

        def run():
            _lib.check(L.o3dmi_nns_hybrid_search_k1(
                h, _lib.ptr(q), b * n, _lib.ptr(idx), _lib.ptr(d2),
                _lib.ptr(cnt), stream()), "k1")
    ms, runs = timed(run, calls)
    torch.cuda.synchronize()
    L.o3dmi_nns_destroy(h)
    print(json.dumps(dict(leg=name, points=n, queries=b * n, calls=calls + 1,
                          wall_ms=ms, runs_ms=runs)))


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
    for n in (5000, 20000):
        t = {}
        for name, kernel in (("score", "ScoreKernel"),
                             ("k1", "HybridSearchK1Kernel")):
            sub = os.path.join(d, "%s_%d" % (name, n))
            with open(sub + ".json") as f:
                info = json.loads(f.read().strip().splitlines()[-1])
            ks = [ns for k, ns in kernel_rows(sub)
                  if kernel in k and "Final" not in k and "Corres" not in k]
            ks = ks[1:] or ks                      # first launch: warm-up
            us = float(np.median(ks)) / 1e3
            t[name] = dict(kernel=kernel, launches=len(ks) + 1,
                           kernel_us_median=us,
                           queries_per_s=info["queries"] / (us * 1e-6),
                           wall_ms=info["wall_ms"])
        t["score_over_k1_rate"] = (t["score"]["queries_per_s"] /
                                   t["k1"]["queries_per_s"])
        sub = os.path.join(d, "operator_%d" % n)
        with open(sub + ".json") as f:
            info = json.loads(f.read().strip().splitlines()[-1])
        ks = [(k, ns) for k, ns in kernel_rows(sub) if "o3dmi" in k]
        wall_ns = sum(info["runs_ms"]) * 1e6   # the 5 timed calls
        per_call = len(ks) / info["calls"]
        kernel_ns = sum(ns for _, ns in ks) / info["calls"]
        t["operator_92pct_random"] = dict(
            rounds=info["rounds"], iterations_run=info["iterations_run"],
            launches_per_call=per_call,
            kernel_ms_per_call=kernel_ns / 1e6,
            wall_ms_under_trace=info["wall_ms"],
            kernel_share_of_wall=kernel_ns / (wall_ns / 5))
        trace[str(n)] = t
    res["kernel_trace"] = trace
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(trace))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "ransac_bench.json"))
    ap.add_argument("--leg", choices=["score", "k1", "operator"])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--merge", help="directory of the per-leg trace runs")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.points)
    if a.merge:
        return merge(a.merge, a.out)
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32",
               seed=0, nproc=os.cpu_count(),
               cases=[case(5000, 100), case(20000, 200)])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
