"""Timing leg of VoxelBlockGrid.extract_triangle_mesh beside
extract_point_cloud on the same grids, with the byte model (tsdf + weight of
the active blocks read once, plus the outputs written).

    python tools/bench_mesh.py [--nx 1024 --ny 512] [--reps 5]

Grids: analytic, one layer of nx x ny blocks of 16^3 (a wavy surface through
every block; default 524 288 blocks), and a small one of 64 x 64 blocks.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open3d_amd import geometry  # noqa: E402


def analytic_grid(nx, ny, res=16):
    g = geometry.VoxelBlockGrid(["tsdf", "weight"],
                                [torch.float32, torch.float32], [1, 1],
                                voxel_size=0.01, block_resolution=res,
                                block_count=nx * ny + 4096)
    j, i = torch.meshgrid(torch.arange(ny, device="cuda"),
                          torch.arange(nx, device="cuda"), indexing="ij")
    keys = torch.stack([i.reshape(-1), j.reshape(-1),
                        torch.zeros_like(i.reshape(-1))], 1).int()
    r3, chunk = res ** 3, 16384
    for s in range(0, keys.shape[0], chunk):
        k = keys[s:s + chunk].contiguous()
        z = torch.zeros(k.shape[0] * r3, device="cuda")
        g.merge_blocks(k, [z, z.clone()])
    tsdf = g.attribute("tsdf").view(-1, r3)
    wgt = g.attribute("weight").view(-1, r3)
    hm = g.hashmap()
    act = hm.active_buf_indices().long()
    kt = hm.key_tensor()
    v = torch.arange(r3, device="cuda")
    lx, ly, lz = v % res, (v // res) % res, v // (res * res)
    for s in range(0, act.shape[0], chunk):
        a = act[s:s + chunk]
        k = kt[a].long()
        X = (k[:, :1] * res + lx).float()
        Y = (k[:, 1:2] * res + ly).float()
        Z = (k[:, 2:] * res + lz).float()
        tsdf[a] = (Z - 7.5 - 3.0 * torch.sin(X * 0.21) *
                   torch.cos(Y * 0.17)) / 8.0
        wgt[a] = 10.0
    torch.cuda.synchronize()
    return g


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], out


def leg(name, g, reps):
    n = g.hashmap().size()
    r3 = g.block_resolution ** 3
    ms_mesh, m = timed(lambda: g.extract_triangle_mesh(3.0), reps)
    ms_pcd, p = timed(lambda: g.extract_point_cloud(3.0), reps)
    nv, nt = m["positions"].shape[0], m["indices"].shape[0]
    read = n * r3 * (4 + 4)
    mesh_bytes = read + nv * 24 + nt * 12
    pcd_bytes = read + p["positions"].shape[0] * 24
    return {"grid": name, "blocks": n, "vertices": nv, "triangles": nt,
            "points": p["positions"].shape[0],
            "mesh_ms": round(ms_mesh, 3), "point_cloud_ms": round(ms_pcd, 3),
            "mesh_over_point_cloud": round(ms_mesh / ms_pcd, 2),
            "byte_model_mesh_GB": round(mesh_bytes / 1e9, 3),
            "byte_model_point_cloud_GB": round(pcd_bytes / 1e9, 3),
            "mesh_GBps_of_model": round(mesh_bytes / ms_mesh / 1e6, 1),
            "point_cloud_GBps_of_model": round(pcd_bytes / ms_pcd / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1024)
    ap.add_argument("--ny", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    legs = [leg("analytic_64x64", analytic_grid(64, 64), a.reps)]
    torch.cuda.empty_cache()
    legs.append(leg("analytic_%dx%d" % (a.nx, a.ny),
                    analytic_grid(a.nx, a.ny), a.reps))
    print(json.dumps({"bench": "extract_triangle_mesh", "legs": legs}))


if __name__ == "__main__":
    main()
