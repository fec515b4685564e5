"""TriangleMesh clean-up, filters and vertex clustering on one MI355X ->
profiles/trianglemesh_clean_bench.json.

    python tools/bench_trianglemesh_clean.py [--out profiles/...json]

Input: the room mesh of tools/bench_trianglemesh.py (marching cubes of the
synthetic room with 300 floating tetrahedra) at about 200 k and about 2 M
triangles, Float32 positions / normals / colours, Int32 indices. Warm, the
median of 10 event-timed calls each, every call with its range check, its pool
allocations and its final wait:
  * remove_duplicated_vertices (beside torch.unique(dim=0) on the positions,
    which sorts and keeps no first occurrence), remove_duplicated_triangles,
    remove_degenerate_triangles;
  * compute_adjacency_list (count, then fill);
  * the four filters at upstream's default arguments, scope All (beside a
    torch restatement of one laplacian pass: index_add_ over the directed
    edges, float atomics, so not the same bits);
  * simplify_vertex_clustering, Average and Quadric, at 2 and 4 times the
    grid's voxel size.
Kernel times come from a run of their own under the kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR/CASE -o t -- \\
        python tools/bench_trianglemesh_clean.py --case CASE --traced
    python tools/bench_trianglemesh_clean.py --merge DIR
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_trianglemesh as bt  # noqa: E402
from open3d_amd import trianglemesh as tm  # noqa: E402

CASES = bt.CASES
# the library's kernels of these calls, by a part of their name
OURS = ("Rep", "RankOfRep", "NonDegenerate", "CompactTriangles", "EdgeRun",
        "UniqueEdges", "Adjacency", "ByHiPairs", "Filter", "LongLists",
        "Widen", "Narrow", "VoxelIndices", "ClusterPairs", "TrianglePlanes",
        "Contract", "MapClusterTriangles", "CheckTriangles", "FiniteCheck",
        "MinMax", "Pair", "Scan", "Prefix", "SlotKeys", "CornerPairs",
        "TriangleAreasF64", "FlagsToMask", "Remap", "Select", "Compact")


def plain_mesh(mesh):
    """positions, indices and the {V,3} normals / colours of their dtype."""
    p = mesh["positions"]
    out = {"positions": p, "indices": mesh["indices"]}
    for name in ("normals", "colors"):
        a = mesh.get(name)
        if a is not None and a.shape == p.shape:
            out[name] = a.to(p.dtype).contiguous()
    return out


def legs_of(mesh, voxel):
    legs = {
        "remove_duplicated_vertices":
            lambda: tm.remove_duplicated_vertices(mesh),
        "remove_duplicated_triangles":
            lambda: tm.remove_duplicated_triangles(mesh),
        "remove_degenerate_triangles":
            lambda: tm.remove_degenerate_triangles(mesh),
        "compute_adjacency_list": lambda: tm.compute_adjacency_list(mesh),
        "filter_sharpen": lambda: tm.filter_sharpen(mesh),
        "filter_smooth_simple": lambda: tm.filter_smooth_simple(mesh),
        "filter_smooth_laplacian": lambda: tm.filter_smooth_laplacian(mesh),
        "filter_smooth_taubin": lambda: tm.filter_smooth_taubin(mesh),
    }
    for name, code in (("average", 0), ("quadric", 1)):
        for k in (2, 4):
            legs["cluster_%s_%dx" % (name, k)] = \
                lambda k=k, code=code: tm.simplify_vertex_clustering(
                    mesh, k * voxel, code)
    return legs


def torch_laplacian_pass(p, edges, lam=0.5):
    """One FilterSmoothLaplacian pass on the positions from directed edges
    {E,2} int64 with index_add_."""
    a, b = edges[:, 0], edges[:, 1]
    w = 1.0 / ((p[a] - p[b]).norm(dim=1) + 1e-12)
    total = torch.zeros(p.shape[0], dtype=p.dtype, device=p.device)
    total.index_add_(0, a, w)
    acc = torch.zeros_like(p)
    acc.index_add_(0, a, w[:, None] * p[b])
    ok = total > 0
    out = p.clone()
    out[ok] = p[ok] + lam * (acc[ok] / total[ok][:, None] - p[ok])
    return out


def case(name, traced):
    cfg, mesh = bt.build_case(name)
    mesh = plain_mesh(mesh)
    p, t = mesh["positions"], mesh["indices"]
    res = dict(cfg, vertices=p.shape[0], triangles=t.shape[0],
               attributes=sorted(mesh))
    out = {}
    for leg, fn in legs_of(mesh, cfg["voxel"]).items():
        def run():
            out["value"] = fn()
        ms, _ = bt.timed(run)
        res[leg] = {"ms": ms}
        value = out["value"]
        if isinstance(value, dict):
            res[leg].update(vertices_out=int(value["positions"].shape[0]),
                            triangles_out=int(value["indices"].shape[0]))
        else:
            res[leg].update(entries=int(value[1].shape[0]))
    if traced:
        return res
    ms, _ = bt.timed(lambda: torch.unique(p, dim=0))
    res["remove_duplicated_vertices"]["torch_unique_dim0_ms"] = ms
    splits, nbrs = tm.compute_adjacency_list(mesh)
    rows = torch.repeat_interleave(
        torch.arange(p.shape[0], device="cuda"), splits[1:] - splits[:-1])
    edges = torch.stack([rows, nbrs.long()], dim=1)
    ms, _ = bt.timed(lambda: torch_laplacian_pass(p, edges))
    ours = tm.filter_smooth_laplacian(mesh, 1, 0.5, tm.FilterScope.Vertex)
    ref = torch_laplacian_pass(p, edges)
    res["filter_smooth_laplacian"].update(
        torch_index_add_pass_ms=ms,
        torch_note="one pass on the positions from a prebuilt edge list; "
                   "ours: adjacency build, positions, normals and colours",
        max_abs_diff_to_torch=float((ours["positions"] - ref).abs().max()))
    return res


def merge(d, out_path):
    """Per case: launches and time per kernel name of the library's kernels
    in the traced run (every leg CALLS + 1 times, mesh set-up included for the
    kernels it shares)."""
    with open(out_path) as f:
        res = json.load(f)
    trace = {}
    for name in CASES:
        sub = os.path.join(d, name)
        if not os.path.isdir(sub):
            continue
        per = {}
        for k, ns in bt.kernel_rows(sub):
            k = bt.short(k)
            if k.startswith("Mesh") or not any(tag in k for tag in OURS):
                continue
            e = per.setdefault(k, [0, 0])
            e[0] += 1
            e[1] += ns
        trace[name] = {k: dict(launches=c, total_us=ns / 1e3,
                               avg_us=ns / 1e3 / c)
                       for k, (c, ns) in sorted(per.items())}
    res["kernel_trace"] = dict(
        note="launch counts and kernel time of the whole traced process per "
             "kernel name; every leg runs %d times" % (bt.CALLS + 1),
        cases=trace)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: len(v) for k, v in trace.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "trianglemesh_clean_bench.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--traced", action="store_true",
                    help="the legs alone, for a kernel-trace run")
    ap.add_argument("--merge", help="directory of the traced runs")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    names = [a.case] if a.case else list(CASES)
    if a.traced:
        print(json.dumps({n: case(n, True) for n in names}))
        return
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32/int32",
               calls=bt.CALLS, timing="median of event-timed calls, ms",
               cases={n: case(n, False) for n in names})
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
