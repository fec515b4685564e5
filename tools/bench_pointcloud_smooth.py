"""PointCloud smoothing and boundary detection on voxel-down-sampled surfaces
of about 100 k and 1 M Float32 points -> profiles/pointcloud_smooth_bench.json.
Warm, event-timed medians of 20 calls, host waits included; the repetitions
of the two sides alternate (fused, chain, fused, chain, ...), so that clock or
thermal drift meets both alike.

For each operator at upstream's defaults (radius 0.05 = 5 voxels here):

  fused   the library call: the search's own wave reduces the neighbour list
          it has just found, no {N,k} table exists
  chain   what a seam-by-seam port would run: the existing search writes
          {N,k} indices + distances (+ counts) to memory, then a table-reading
          kernel (the same per-point body) reads them back

  laplacian  10 iterations, lambda 0.5, max_nn 20, re-searched neighbourhoods:
             per pass o3dmi_nns_knn_search into {N,21} + the table pass
  taubin     the same with mu -0.53 (20 passes)
  mls        radius 0.05, max_nn 30: index + o3dmi_nns_hybrid_search + table
  bilateral  radius 0.05, max_nn 30, sigma_s = sigma_r = 0.05: the same
  boundary   radius 0.05, max_nn 30, 90 degrees: hybrid search +
             o3dmi_pointcloud_boundary_from_neighbors

Both sides are this project's code, so the ratio is a record, not a pass
mark. Outputs of the two are compared (they run the same statements: 0
differing rows expected). Kernel times come from a run of their own:

    python tools/bench_pointcloud_smooth.py [--sizes 150000 1500000] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- \\
        python tools/bench_pointcloud_smooth.py --only mls --reps 3 --out /dev/null
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from open3d_amd import _lib, pointcloud, registration, synthetic  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

VOXEL = 0.01
RADIUS, MAX_NN, SIGMA = 0.05, 30, 0.05
ITERATIONS, LAMBDA, MU, LAPLACIAN_NN = 10, 0.5, -0.53, 20
LAPLACIAN, MLS, BILATERAL, BOUNDARY = 0, 1, 2, 3  # SmoothOpKind
OPERATORS = ("laplacian", "taubin", "mls", "bilateral", "boundary")


def _once(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def timed_pair(first, second, reps):
    """Both warmed, then `reps` rounds of (first, second)."""
    for fn in (first, second):
        fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(_once(first))
        b.append(_once(second))
    return _stats(a), _stats(b)


def _table_op():
    """The internal table-reading seam (csrc/pointcloud_smooth.h; bound in
    _lib.INTERNAL_PROTOTYPES)."""
    return _lib.lib().o3dmi_internal_pointcloud_smooth_from_neighbors


def _p(t):
    return _lib.ptr(t) if t is not None else None


class KnnChain:
    """Laplacian / Taubin seam by seam: every pass is o3dmi_nns_knn_search
    into {N,k} indices + distances, then the table pass. The table and the
    two position buffers are allocated once, so that no allocator time is
    counted on this side (the fused call allocates its one output)."""

    def __init__(self, p):
        self.p, self.n = p, p.shape[0]
        self.k = min(self.n, LAPLACIAN_NN + 1)
        self.idx = torch.empty((self.n, self.k), dtype=torch.int32,
                               device="cuda")
        self.d2 = torch.empty((self.n, self.k), dtype=p.dtype, device="cuda")
        self.buf = [torch.empty_like(p), torch.empty_like(p)]

    def run(self, factors):
        L, op, n, k = _lib.lib(), _table_op(), self.n, self.k
        cur, t = self.p, 0
        for _ in range(ITERATIONS):
            for f in factors:
                nxt = self.buf[t & 1]
                _lib.check(L.o3dmi_nns_knn_search(
                    _p(cur), n, _p(cur), n, 0, k, _p(self.idx), _p(self.d2),
                    stream()), "knn_search")
                _lib.check(op(LAPLACIAN, _p(cur), None, _p(self.idx), None,
                              None, n, k, 0, f, 0.0, _p(nxt), None, None,
                              stream()), "table laplacian")
                cur, t = nxt, t + 1
        torch.cuda.synchronize()
        return cur


class HybridTable:
    """Index + o3dmi_nns_hybrid_search into {N, MAX_NN} buffers."""

    def __init__(self, p):
        self.p, self.n = p, p.shape[0]
        self.idx = torch.empty((self.n, MAX_NN), dtype=torch.int32,
                               device="cuda")
        self.d2 = torch.empty((self.n, MAX_NN), dtype=p.dtype, device="cuda")
        self.cnt = torch.empty(self.n, dtype=torch.int32, device="cuda")

    def search(self):
        L = _lib.lib()
        index = C.c_void_p()
        _lib.check(L.o3dmi_nns_create(_p(self.p), self.n, 0,
                                      C.c_double(RADIUS), stream(),
                                      C.byref(index)), "nns_create")
        st = L.o3dmi_nns_hybrid_search(index, _p(self.p), self.n, MAX_NN,
                                       _p(self.idx), _p(self.d2),
                                       _p(self.cnt), stream())
        return index, st


def chain_hybrid(table, kind, nrm, p0, p1):
    p, n = table.p, table.n
    index, st = table.search()
    try:
        _lib.check(st, "hybrid_search")
        out = out_n = mask = None
        if kind == BOUNDARY:
            mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
            _lib.check(_lib.lib().o3dmi_pointcloud_boundary_from_neighbors(
                _p(p), _p(nrm), _p(table.idx), _p(table.cnt), n, MAX_NN, 0,
                C.c_double(p0), _p(mask), stream()), "boundary seam")
        else:
            out = p.clone()
            if kind == MLS and nrm is not None:
                out_n = nrm.clone()
            _lib.check(_table_op()(
                kind, _p(p), _p(nrm) if kind == BILATERAL else None,
                _p(table.idx), _p(table.d2), _p(table.cnt), n, MAX_NN, 0, p0,
                p1, _p(out), _p(out_n), None, stream()), "table op")
        torch.cuda.synchronize()
    finally:
        _lib.lib().o3dmi_nns_destroy(index)
    return mask if kind == BOUNDARY else out


def fused_boundary_mask(p, nrm):
    """The mask alone, as the chain returns it (the Python mirror would add
    the SelectByMask compaction to the fused side only)."""
    n = p.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    m = C.c_int64(0)
    _lib.check(_lib.lib().o3dmi_pointcloud_compute_boundary_points(
        _p(p), _p(nrm), n, 0, C.c_double(RADIUS), MAX_NN, C.c_double(90.0),
        _p(mask), C.byref(m), stream()), "compute_boundary_points")
    return mask


def _rows_differing(a, b):
    d = a != b
    return int((d.any(1) if d.dim() > 1 else d).sum())


def bench_size(n_sample, reps, only):
    pair = synthetic.make_icp_pair(1000, n_sample, seed=1)
    p, nrm = registration.voxel_down_sample(
        torch.from_numpy(pair["target"]).cuda(),
        torch.from_numpy(pair["target_normals"]).cuda(), VOXEL)
    n = p.shape[0]
    cloud = {"positions": p, "normals": nrm}
    bare = {"positions": p}
    table = HybridTable(p)
    knn = KnnChain(p)
    out = dict(points=n, voxel=VOXEL, radius=RADIUS,
               chain_table_bytes_hybrid=n * MAX_NN * 8 + n * 4,
               chain_table_bytes_knn_per_pass=n * (LAPLACIAN_NN + 1) * 8)
    cases = {
        "laplacian": (
            lambda: pointcloud.smooth_laplacian(
                bare, ITERATIONS, LAMBDA, LAPLACIAN_NN)["positions"],
            lambda: knn.run((LAMBDA,))),
        "taubin": (
            lambda: pointcloud.smooth_taubin(
                bare, ITERATIONS, LAMBDA, MU, LAPLACIAN_NN)["positions"],
            lambda: knn.run((LAMBDA, MU))),
        "mls": (
            lambda: pointcloud.smooth_mls(bare, RADIUS, MAX_NN)["positions"],
            lambda: chain_hybrid(table, MLS, None, RADIUS, 0.0)),
        "bilateral": (
            lambda: pointcloud.smooth_bilateral(
                cloud, RADIUS, MAX_NN, SIGMA, SIGMA)["positions"],
            lambda: chain_hybrid(table, BILATERAL, nrm, SIGMA, SIGMA)),
        "boundary": (
            lambda: fused_boundary_mask(p, nrm),
            lambda: chain_hybrid(table, BOUNDARY, nrm, 90.0, 0.0)),
    }
    for name in OPERATORS:
        if name not in only:
            continue
        fused_fn, chain_fn = cases[name]
        fused, chain = timed_pair(fused_fn, chain_fn, reps)
        out[name] = dict(
            fused=fused, chain=chain,
            chain_over_fused=chain["median_ms"] / fused["median_ms"],
            rows_differing=_rows_differing(fused_fn(), chain_fn()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+",
                    default=[150000, 1500000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", nargs="+", default=list(OPERATORS),
                    choices=OPERATORS)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "pointcloud_smooth_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud_smooth: no GPU; nothing is "
                         "measured without one")
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32",
               reps=args.reps,
               cases=[bench_size(s, args.reps, args.only)
                      for s in args.sizes])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
