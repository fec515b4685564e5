"""The non-rigid SLAC optimizer on one MI355X ->
profiles/slac_nonrigid_bench.json.

    python tools/bench_slac_nonrigid.py [--out profiles/slac_nonrigid_bench.json]

Scene: tests/_slac_nonrigid_oracle.make_scene at 60 k samples (3 fragments of
about 22 k points, 3 edges), control grids of about 64, 1000 and 4000 nodes
(grid sizes 1.0, 0.19, 0.097). Float32 fragments, warm, median of 3,
device-synchronised wall times. Per grid:

  iteration   o3dmi_slac_optimize with 2 iterations minus with 1: zeroing the
              float64 system, the one-launch alignment fill, pose blocks,
              regularizer, pin, Cholesky, downloads and the two updates
  solve       o3dmi_slac_solve_spd alone on a diagonally dominant matrix of
              the same n
  fill        iteration - solve (derived, not timed by itself)
  seam        upstream's shape: one o3dmi_fill_in_slac_alignment_term per edge
              and one o3dmi_fill_in_slac_regularizer_term into a float32
              {n,n} system indexed by raw buffer index (n = 6 N + 3 capacity);
              the per-edge gathers, Parameterize, Deform and transforms a
              dispatcher issues before each call are prepared outside the
              timed region

and the deviations from the numpy oracle that tests/test_slac_nonrigid_gpu.py
asserts at 16 x (regularizer seam; the driver with the anchor pinned).
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
from open3d_amd import slac  # noqa: E402
import _slac_nonrigid_oracle as no  # noqa: E402

GRID_SIZES = [1.0, 0.19, 0.097]
THRESHOLD = 0.07
F = np.float32


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def timed(fn, repeat=3):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def optimize_ms(fc, start, edges, grid_size, iterations):
    params = slac.SLACOptimizerParams(max_iterations=iterations)
    out = {}

    def run():
        grid = slac.ControlGrid(grid_size, 8000)
        st, _, info = slac.slac_optimize_raw(fc, start, edges, params, grid)
        assert st == 0, st
        out.update(info, nodes=grid.size())
    return timed(run), out


def solve_ms(n):
    g = torch.Generator(device="cuda").manual_seed(n)
    A = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=g)
    A = torch.tril(A) + torch.diag(torch.full((n,), float(n),
                                              dtype=torch.float64,
                                              device="cuda"))
    b = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    L, x = torch.empty_like(A), torch.empty_like(b)

    def run():
        L.copy_(A)
        x.copy_(b)
        assert slac.solve_spd_raw(L, x) == 0
    copy = timed(lambda: (L.copy_(A), x.copy_(b)))
    return timed(run) - copy


def transform(T, x, with_t=True):
    T = torch.from_numpy(np.asarray(T, np.float64).astype(F)).cuda()
    y = x @ T[:3, :3].T
    return (y + T[:3, 3]).contiguous() if with_t else y.contiguous()


def seam_ms(fc, start, edges, grid_size):
    """-> (ms, n_vars)."""
    grid = slac.ControlGrid(grid_size, 8000)
    for p, _ in fc:
        grid.touch(p)
    grid.compactify()
    N = len(fc)
    cap = grid.get_hashmap().capacity()
    n = 6 * N + 3 * cap
    calls = []
    for i, j, T_ij in edges:
        cs = slac.get_correspondence_set_for_point_cloud_pair(
            i, j, fc[i][0], fc[j][0], start[i], start[j], T_ij, THRESHOLD, 0.3)
        pi = grid.parameterize(fc[i][0][cs[:, 0]], fc[i][1][cs[:, 0]])
        pj = grid.parameterize(fc[j][0][cs[:, 1]], fc[j][1][cs[:, 1]])
        assert pi.positions.shape[0] == pj.positions.shape[0] == cs.shape[0]
        Cp, Cn, _ = grid.deform(pi)
        Cq, _, _ = grid.deform(pj)
        Ri_Cn = transform(start[i], Cn, False)
        Rj = torch.from_numpy(np.asarray(start[j])[:3, :3].astype(F)).cuda()
        calls.append((transform(start[i], Cp), transform(start[j], Cq), Cn,
                      Ri_Cn, (Ri_Cn @ Rj).contiguous(), pi.Grid8NbIndices,
                      pj.Grid8NbIndices, pi.Grid8NbVertexInterpRatios,
                      pj.Grid8NbVertexInterpRatios, i, j, N, THRESHOLD))
    active, nb, masks = grid.get_neighbor_grid_map()
    init, curr = grid.get_init_positions(), grid.get_curr_positions()
    AtA = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    Atb = torch.zeros(n, dtype=torch.float32, device="cuda")
    res = torch.zeros(1, dtype=torch.float32, device="cuda")

    def run():
        AtA.zero_()
        Atb.zero_()
        for c in calls:
            slac.fill_in_slac_alignment_term(AtA, Atb, res, *c)
        slac.fill_in_slac_regularizer_term(AtA, Atb, res, active, nb, masks,
                                           init, curr, float(N), N,
                                           grid.get_anchor_idx())
    return timed(run), n


def deviations():
    """The figures tests/test_slac_nonrigid_gpu.py asserts at 16 x."""
    import test_slac_nonrigid_gpu as tg
    reg = {name: tg.regularizer_deviation(name, g, curr, masks)[0]
           for name, g, curr, masks in no.regularizer_cases()}
    frags, start, edges, ogrid = no.scene()
    want = no.oracle_run(3, pin_anchor=True)
    lu = no.oracle_run(3)
    st, P, info, grid = tg.gpu_run(3)
    assert st == 0
    nodes = tg.nodes_by_key(grid)
    curr = np.array([nodes[tuple(int(v) for v in k)] for k in ogrid.keys], F)
    al = np.array(want["alignment_losses"])
    return dict(
        regularizer_seam_max_relative_deviation=reg,
        driver=dict(
            scene="3 fragments x ~4000 points, %d nodes, 3 iterations, "
                  "oracle with the anchor pinned" % len(ogrid.keys),
            pose_deviation=float(np.abs(P - np.stack(want["poses"])).max()),
            node_deviation_m=float(np.abs(curr - want["curr"]).max()),
            alignment_loss_relative_deviation=(
                np.abs(info["alignment_losses"] - al) / al).tolist(),
            alignment_losses=info["alignment_losses"].tolist(),
            regularizer_losses=info["regularizer_losses"].tolist(),
            lu_oracle_pose_deviation=float(
                np.abs(P - np.stack(lu["poses"])).max()),
            lu_oracle_node_deviation_m=float(
                np.abs(curr - lu["curr"]).max()),
            lu_oracle_alignment_losses=lu["alignment_losses"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "slac_nonrigid_bench.json"))
    args = ap.parse_args()
    frags, start, edges = no.make_scene(n_sample=60000)
    fc = [(cuda(p), cuda(n)) for p, n in frags]
    res = dict(device=torch.cuda.get_device_name(0),
               fragments=[int(f[0].shape[0]) for f in frags],
               edges=len(edges), timing="wall ms, warm, median of 3",
               grids=[])
    for gs in GRID_SIZES:
        one, info = optimize_ms(fc, start, edges, gs, 1)
        two, _ = optimize_ms(fc, start, edges, gs, 2)
        G = info["nodes"]
        n = 6 * len(fc) + 3 * G
        solve = solve_ms(n)
        seam, n_seam = seam_ms(fc, start, edges, gs)
        row = dict(grid_size=gs, nodes=G, n=n,
                   correspondences=int(sum(c for c, k in zip(
                       info["n_corres"], info["kept"]) if k)),
                   optimize_1_iteration_ms=one, optimize_2_iterations_ms=two,
                   iteration_ms=two - one, solve_ms=solve,
                   fill_ms_derived=two - one - solve,
                   seam_by_seam_fill_ms=seam, seam_n_vars=n_seam)
        print(json.dumps(row), flush=True)
        res["grids"].append(row)
    res.update(deviations())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
