"""TriangleMesh sampling, closest points and ComputeMetrics on one MI355X ->
profiles/mesh_distance_bench.json.

    python tools/bench_mesh_distance.py [--out profiles/mesh_distance_bench.json]

Input: the marching-cubes mesh of the synthetic room (tools/
bench_trianglemesh.py builds it) at about 200 k and about 2 M triangles.
Float32 positions, Int32 indices, warm, the median of 10 event-timed calls:
  * build: o3dmi_mesh_bvh_create (range and finiteness checks, scene box,
    Morton codes, pair sort, radix tree, refit, the final wait);
  * query: o3dmi_internal_mesh_bvh_query for the distance of 100 k and 1 M
    points sampled on the mesh and moved half a voxel off it, with the lanes
    taking the queries in input order and in Morton order (the two variants
    DESIGN 4m compares), the inner nodes opened and triangles tested per
    query, the bytes those stand for (64 per node, 48 per triangle), and
    beside them o3dmi_pointcloud_nearest_distance of the same queries against
    the mesh's vertices: the nearest sibling on this hardware, not a pass
    mark;
  * sample: o3dmi_trianglemesh_sample_points_uniformly alone, 100 k and 1 M
    points;
  * metrics: o3dmi_trianglemesh_compute_metrics of the mesh against itself
    moved half a voxel, at upstream's default n_sampled_points = 1000.
Every call includes its checks, its pool allocations and its final wait. The
rates are recorded, not a pass mark. Kernel times of the build come from a
run of its own under the kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR/CASE_build -o t -- \\
        python tools/bench_mesh_distance.py --case CASE --leg build \\
        > DIR/CASE_build.json
    python tools/bench_mesh_distance.py --merge DIR
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
from open3d_amd import _lib  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

CASES = bt.CASES
QUERY_COUNTS = {"100k": 100000, "1M": 1000000}
NODE_BYTES, LEAF_BYTES = 64, 48
METRICS_SAMPLES = 1000  # MetricParameters' default


class Legs:
    def __init__(self, mesh, voxel):
        self.p = mesh["positions"].contiguous()
        self.t = mesh["indices"].contiguous()
        self.v, self.m = self.p.shape[0], self.t.shape[0]
        self.voxel = voxel
        self.L = _lib.lib()
        self.args = (_lib.ptr(self.p), self.v, _lib.F32, _lib.ptr(self.t),
                     self.m, _lib.I32)

    def create(self):
        h = C.c_void_p()
        _lib.check(self.L.o3dmi_mesh_bvh_create(*self.args, C.byref(h),
                                                stream()), "mesh_bvh_create")
        return h

    def build(self):
        def run():
            self.L.o3dmi_mesh_bvh_destroy(self.create())
        ms, _ = bt.timed(run)
        return {"ms": ms, "triangles_per_s": self.m / ms * 1e3}

    def samples(self, n, seed=0):
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        _lib.check(self.L.o3dmi_trianglemesh_sample_points_uniformly(
            *self.args, n, seed, None, None, None, 0, _lib.ptr(out), None,
            None, None, stream()), "sample_points_uniformly")
        return out

    def sample(self):
        res = {}
        for name, n in QUERY_COUNTS.items():
            ms, _ = bt.timed(lambda: self.samples(n))
            res[name] = {"ms": ms, "points_per_s": n / ms * 1e3}
        return res

    def query(self):
        h = self.create()
        res = {}
        for name, n in QUERY_COUNTS.items():
            q = (self.samples(n) + 0.5 * self.voxel).contiguous()
            dist = torch.empty(n, dtype=torch.float32, device="cuda")
            entry = {}
            for order, key in ((0, "input_order"), (1, "morton_order")):
                visits = (C.c_uint64 * 2)()

                def run(count=None):
                    _lib.check(self.L.o3dmi_internal_mesh_bvh_query(
                        h, _lib.ptr(q), n, None, None, None, None,
                        _lib.ptr(dist), order, count, stream()),
                        "mesh_bvh_query")
                ms, _ = bt.timed(run)
                run(visits)
                per_query = (visits[0] * NODE_BYTES +
                             visits[1] * LEAF_BYTES) / n
                entry[key] = {
                    "ms": ms, "queries_per_s": n / ms * 1e3,
                    "nodes_opened_per_query": visits[0] / n,
                    "triangles_tested_per_query": visits[1] / n,
                    "bytes_per_query": per_query,
                    "bytes_per_s_if_uncached": per_query * n / ms * 1e3}
            idx_dist = torch.empty(n, dtype=torch.float32, device="cuda")
            ms, _ = bt.timed(lambda: _lib.check(
                self.L.o3dmi_pointcloud_nearest_distance(
                    _lib.ptr(self.p), self.v, _lib.ptr(q), n, _lib.F32,
                    _lib.ptr(idx_dist), None, stream()), "nearest_distance"))
            entry["nearest_vertex_sibling"] = {
                "ms": ms, "queries_per_s": n / ms * 1e3,
                "mean_distance": float(idx_dist.mean()),
                "mean_mesh_distance": float(dist.mean())}
            res[name] = entry
        self.L.o3dmi_mesh_bvh_destroy(h)
        return res

    def metrics(self):
        p2 = (self.p + 0.5 * self.voxel).contiguous()
        codes = (C.c_int * 3)(0, 1, 2)
        radii = (C.c_float * 1)(self.voxel)
        values = (C.c_float * 3)()

        def run():
            _lib.check(self.L.o3dmi_trianglemesh_compute_metrics(
                _lib.ptr(self.p), self.v, _lib.ptr(self.t), self.m, _lib.I32,
                _lib.ptr(p2), self.v, _lib.ptr(self.t), self.m, _lib.I32,
                _lib.F32, codes, 3, radii, 1, METRICS_SAMPLES, 0, values, 3,
                None, stream()), "compute_metrics")
        ms, _ = bt.timed(run)
        return {"ms": ms, "n_sampled_points": METRICS_SAMPLES,
                "values": list(values)}


LEGS = ["build", "sample", "query", "metrics"]


def build_case(name):
    cfg = CASES[name]
    mesh = bt.room_mesh(cfg["voxel"], cfg["frames"], cfg["block_count"])
    return cfg, Legs(mesh, cfg["voxel"])


def case(name):
    cfg, legs = build_case(name)
    res = dict(cfg, vertices=legs.v, triangles=legs.m)
    for leg_name in LEGS:
        res[leg_name] = getattr(legs, leg_name)()
    return res


def leg(case_name, leg_name):
    """One leg for a kernel-trace run of its own; prints one JSON line."""
    _, legs = build_case(case_name)
    torch.cuda.synchronize()
    res = getattr(legs, leg_name)()
    print(json.dumps(dict(case=case_name, leg=leg_name, calls=bt.CALLS + 1,
                          triangles=legs.m, result=res)))


OURS = ("SceneBox", "TriangleCodes", "Leaves", "RadixTree", "Refit", "Pair",
        "CheckTriangles", "CheckFinite", "Finite", "ClosestPoint",
        "QueryCodes")


def merge(d, out_path):
    with open(out_path) as f:
        res = json.load(f)
    trace = {}
    for case_name in CASES:
        sub = os.path.join(d, "%s_build" % case_name)
        if not os.path.exists(sub + ".json"):
            continue
        with open(sub + ".json") as f:
            info = json.loads(f.read().strip().splitlines()[-1])
        per = {}
        for k, ns in bt.kernel_rows(sub):
            k = bt.short(k)
            if k.startswith("Mesh") or not any(tag in k for tag in OURS):
                continue
            e = per.setdefault(k, [0, 0])
            e[0] += 1
            e[1] += ns
        trace[case_name] = dict(
            wall_ms_under_trace=info["result"]["ms"], calls=info["calls"],
            kernels={k: dict(launches=c, total_us=ns / 1e3,
                             avg_us=ns / 1e3 / c)
                     for k, (c, ns) in sorted(per.items())})
    res["build_kernel_trace"] = trace
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: sorted(v["kernels"]) for k, v in trace.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "mesh_distance_bench.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--merge", help="directory of the build trace runs")
    a = ap.parse_args()
    if a.leg:
        return leg(a.case or "200k", a.leg)
    if a.merge:
        return merge(a.merge, a.out)
    names = [a.case] if a.case else list(CASES)
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32/int32",
               calls=bt.CALLS, timing="median of event-timed calls, ms",
               note="rates are recorded, not a pass mark",
               cases={n: case(n) for n in names})
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
