"""The ray queries on a mesh (CastRays, TestOcclusions, ComputeOccupancy,
ComputeSignedDistance) on one MI355X -> profiles/mesh_raycast_bench.json.

    python tools/bench_mesh_raycast.py [--out profiles/mesh_raycast_bench.json]

Input: the marching-cubes mesh of the synthetic room of tools/
bench_mesh_distance.py at about 200 k and about 2 M triangles. Float32, warm,
the median of 10 event-timed calls on one handle:
  * cast: o3dmi_internal_mesh_bvh_ray_query (closest hit) of a 640x480 and a
    1280x720 pinhole view from inside the room (coherent rays) and of 1 M rays
    from points half a voxel off the mesh in random directions (incoherent),
    with the lanes taking the rays in input order and in the Morton order of
    their origins, the inner nodes opened and triangles tested per ray, and
    the any-hit query (TestOcclusions) of the same rays;
  * vote: o3dmi_mesh_bvh_compute_occupancy / _compute_signed_distance of 100 k
    and 1 M points at nsamples 1 and 3, and beside the fused vote the chain a
    seam-by-seam port would run (the {nsamples q, 6} ray tensor ->
    count_intersections -> the vote in torch), asserted to give the same
    bits.
Every call includes its checks, its pool allocations and its final wait. The
rates are recorded, not a pass mark. The one ratio worth stating, the
closest-hit kernel beside ClosestPointKernel on the same tree and the same
1 M origins, comes from a run of its own under the kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR/CASE_ratio -o t -- \\
        python tools/bench_mesh_raycast.py --case CASE --leg ratio \\
        > DIR/CASE_ratio.json
    python tools/bench_mesh_raycast.py --merge DIR
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_trianglemesh as bt  # noqa: E402
from open3d_amd import _lib, synthetic  # noqa: E402
from open3d_amd import trianglemesh as tm  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

CASES = bt.CASES
VIEWS = {"640x480": (640, 480), "1280x720": (1280, 720)}
VIEW_FRAME = 7  # between the integrated frames 5 and 10
N_RANDOM = 1000000
POINT_COUNTS = {"100k": 100000, "1M": 1000000}
NSAMPLES = (1, 3)
CLOSEST, ANY = 0, 1
INF = float("inf")


class Legs:
    def __init__(self, mesh, voxel):
        self.mesh = {"positions": mesh["positions"].contiguous(),
                     "indices": mesh["indices"].contiguous()}
        self.m = self.mesh["indices"].shape[0]
        self.voxel = voxel
        self.L = _lib.lib()
        self.bvh = tm.MeshBVH(self.mesh)
        self.h = self.bvh._handle

    def origins(self, n, seed=0):
        """Points sampled on the mesh and moved half a voxel off it."""
        p = tm.sample_points_uniformly(self.mesh, n, seed=seed)["positions"]
        return (p + 0.5 * self.voxel).contiguous()

    def random_rays(self, n):
        g = torch.Generator(device="cuda").manual_seed(1)
        d = torch.randn((n, 3), generator=g, device="cuda",
                        dtype=torch.float32)
        return torch.cat([self.origins(n), d], dim=1).contiguous()

    def ray_sets(self):
        sets = {}
        for name, (w, h) in VIEWS.items():
            rays = tm.create_rays_pinhole(synthetic.intrinsics(w, h),
                                          synthetic.pose(VIEW_FRAME), w, h)
            sets["view_" + name] = rays.reshape(-1, 6).contiguous()
        sets["random_1M"] = self.random_rays(N_RANDOM)
        return sets

    def ray_query(self, kind, rays, order, t_hit, occluded, visits=None):
        _lib.check(self.L.o3dmi_internal_mesh_bvh_ray_query(
            self.h, kind, _lib.ptr(rays), rays.shape[0], 0.0, INF,
            _lib.ptr(t_hit), None, None, None, None, _lib.ptr(occluded), None,
            order, visits, stream()), "mesh_bvh_ray_query")

    def cast(self):
        res = {}
        for name, rays in self.ray_sets().items():
            n = rays.shape[0]
            t_hit = torch.empty(n, dtype=torch.float32, device="cuda")
            occluded = torch.empty(n, dtype=torch.uint8, device="cuda")
            entry = {"rays": n}
            for kind, key in ((CLOSEST, "cast_rays"),
                              (ANY, "test_occlusions")):
                for order, okey in ((0, "input_order"), (1, "morton_order")):
                    visits = (C.c_uint64 * 2)()
                    ms, _ = bt.timed(lambda: self.ray_query(
                        kind, rays, order, t_hit, occluded))
                    self.ray_query(kind, rays, order, t_hit, occluded, visits)
                    entry.setdefault(key, {})[okey] = {
                        "ms": ms, "rays_per_s": n / ms * 1e3,
                        "nodes_opened_per_ray": visits[0] / n,
                        "triangles_tested_per_ray": visits[1] / n}
            entry["hit_fraction"] = float(torch.isfinite(t_hit).float().mean())
            assert bool((torch.isfinite(t_hit) == (occluded != 0)).all())
            res[name] = entry
        return res

    def chain(self, points, nsamples, signed):
        """The seam-by-seam port: ray tensor, counts, the vote in torch."""
        dirs = (C.c_float * (3 * nsamples))()
        _lib.check(self.L.o3dmi_raycast_vote_directions(nsamples, dirs),
                   "vote_directions")
        d = torch.tensor(list(dirs), dtype=torch.float32,
                         device="cuda").reshape(1, nsamples, 3)
        q = points.shape[0]
        rays = torch.cat([points[:, None, :].expand(q, nsamples, 3),
                          d.expand(q, nsamples, 3)], dim=2)
        counts = self.bvh.count_intersections(rays.contiguous())
        inside = (counts % 2).sum(dim=1) > nsamples // 2
        if not signed:
            return inside.to(torch.float32)
        sign = torch.where(inside, -1.0, 1.0).to(torch.float32)
        return self.bvh.compute_distance(points) * sign

    def vote(self):
        res = {}
        for name, n in POINT_COUNTS.items():
            points = self.origins(n, seed=2)
            entry = {}
            for nsamples in NSAMPLES:
                for signed, key in ((False, "compute_occupancy"),
                                    (True, "compute_signed_distance")):
                    fn = self.bvh.compute_signed_distance if signed else \
                        self.bvh.compute_occupancy
                    ms, _ = bt.timed(lambda: fn(points, nsamples))
                    cms, _ = bt.timed(
                        lambda: self.chain(points, nsamples, signed))
                    fused = fn(points, nsamples)
                    chained = self.chain(points, nsamples, signed)
                    assert torch.equal(fused.view(torch.int32),
                                       chained.view(torch.int32)), \
                        "the fused vote and the chain differ"
                    entry["%s_nsamples%d" % (key, nsamples)] = {
                        "ms": ms, "points_per_s": n / ms * 1e3,
                        "chain_ms": cms, "chain_over_fused": cms / ms,
                        "inside_fraction": float(
                            (fused < 0).float().mean() if signed
                            else fused.mean())}
            res[name] = entry
        return res

    def ratio(self):
        """The closest-hit and the closest-point kernels on the same tree and
        origins, for the kernel trace; wall times beside them."""
        rays = self.random_rays(N_RANDOM)
        points = rays[:, :3].contiguous()
        t_hit = torch.empty(N_RANDOM, dtype=torch.float32, device="cuda")
        dist = torch.empty(N_RANDOM, dtype=torch.float32, device="cuda")
        ray_ms, _ = bt.timed(lambda: self.ray_query(CLOSEST, rays, 0, t_hit,
                                                    None))
        point_ms, _ = bt.timed(lambda: _lib.check(
            self.L.o3dmi_internal_mesh_bvh_query(
                self.h, _lib.ptr(points), N_RANDOM, None, None, None, None,
                _lib.ptr(dist), 0, None, stream()), "mesh_bvh_query"))
        return {"cast_rays_ms": ray_ms, "closest_points_ms": point_ms}


LEGS = ["cast", "vote"]


def build_case(name):
    cfg = CASES[name]
    mesh = bt.room_mesh(cfg["voxel"], cfg["frames"], cfg["block_count"])
    return cfg, Legs(mesh, cfg["voxel"])


def case(name):
    cfg, legs = build_case(name)
    res = dict(cfg, triangles=legs.m)
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


def merge(d, out_path):
    with open(out_path) as f:
        res = json.load(f)
    trace = {}
    for case_name in CASES:
        sub = os.path.join(d, "%s_ratio" % case_name)
        if not os.path.exists(sub + ".json"):
            continue
        with open(sub + ".json") as f:
            info = json.loads(f.read().strip().splitlines()[-1])
        per = {}
        for k, ns in bt.kernel_rows(sub):
            k = bt.short(k)
            if "RayQueryKernel" in k or "ClosestPointKernel" in k:
                per.setdefault(k.split("<")[0], []).append(ns / 1e3)
        kernels = {k: dict(launches=len(v), median_us=float(np.median(v)))
                   for k, v in sorted(per.items())}
        entry = dict(wall_ms_under_trace=info["result"], calls=info["calls"],
                     rays=N_RANDOM, kernels=kernels)
        if len(kernels) == 2:
            entry["closest_hit_over_closest_point"] = (
                kernels["RayQueryKernel"]["median_us"] /
                kernels["ClosestPointKernel"]["median_us"])
        trace[case_name] = entry
    res["closest_hit_beside_closest_point_kernel_trace"] = trace
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(trace))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "mesh_raycast_bench.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--leg", choices=LEGS + ["ratio"])
    ap.add_argument("--merge", help="directory of the ratio trace runs")
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
