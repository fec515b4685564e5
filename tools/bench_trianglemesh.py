"""TriangleMesh operators on one MI355X -> profiles/trianglemesh_bench.json.

    python tools/bench_trianglemesh.py [--out profiles/trianglemesh_bench.json]

Input: the marching-cubes mesh of the synthetic room (the grid built as
tools/bench_slam.py --mode extract builds it, then extract_triangle_mesh), at
two voxel sizes chosen for about 200 k and about 2 M triangles, with 300
small floating components (tetrahedra) appended. Float32 positions, Int32
indices, warm, the median of 10 event-timed calls each:
  * sort: o3dmi_sort_pairs_u32 on the 3 m (vertex id, corner) pairs, beside
    torch.sort(stable=True) on the same keys;
  * vertex_normals: o3dmi_trianglemesh_vertex_normals (not normalised), beside
    a torch restatement (cross products, three index_add_ calls: float atomics,
    so not the same bits);
  * edge_table: o3dmi_trianglemesh_get_non_manifold_edges in counting mode
    (the table, the run flags and their scan);
  * cluster: o3dmi_trianglemesh_cluster_connected_triangles with counts and
    areas;
  * select: trianglemesh.select_faces_by_mask keeping the components above 100
    triangles, attribute rows included.
Every call includes its range check, its pool allocations and its final wait.
Kernel times come from runs of their own under the kernel trace, one per leg:

    rocprofv3 --kernel-trace --output-format csv -d DIR/CASE_LEG -o t -- \\
        python tools/bench_trianglemesh.py --case CASE --leg LEG
    python tools/bench_trianglemesh.py --merge DIR
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
from open3d_amd import _lib, geometry, synthetic  # noqa: E402
from open3d_amd import trianglemesh as tm  # noqa: E402
from open3d_amd.core import stream  # noqa: E402

# voxel size, frames, block count: sized on the synthetic room
CASES = {"200k": dict(voxel=0.0065, frames=4, block_count=50000),
         "2M": dict(voxel=0.002, frames=4, block_count=200000)}
LEGS = ["sort", "vertex_normals", "edge_table", "cluster", "select"]
CALLS = 10
N_FLOATING = 300


def room_mesh(voxel, frames, block_count):
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    g = geometry.VoxelBlockGrid(["tsdf", "weight", "color"],
                                [torch.float32, torch.uint16, torch.uint16],
                                [1, 1, 3], voxel, 16, block_count)
    ds, cs, Ts = [], [], []
    for k in range(frames):
        d, c, _, T = synthetic.render_frames(k * 5, 1, W, H, device="cuda")
        ds.append(d[0].contiguous())
        cs.append(c[0].contiguous())
        Ts.append(T[0])
    g.integrate_frames(ds, cs, K, K, Ts, 1000.0, 3.0, 8.0)
    torch.cuda.synchronize()
    mesh = g.extract_triangle_mesh(3.0)
    return {k: v.clone() for k, v in mesh.items()}


def with_floating_components(mesh, n, voxel, seed=0):
    """Appends n tetrahedra (4 vertices, 4 triangles each) around the mesh."""
    rng = np.random.default_rng(seed)
    p = mesh["positions"]
    lo, hi = p.min(0).values.cpu().numpy(), p.max(0).values.cpu().numpy()
    centre = rng.uniform(lo, hi, (n, 1, 3))
    corner = voxel * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    verts = (centre + corner[None]).reshape(-1, 3).astype(np.float32)
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    tris = (faces[None] + 4 * np.arange(n)[:, None, None] +
            p.shape[0]).reshape(-1, 3).astype(np.int32)
    out = {}
    for k, v in mesh.items():
        if k == "indices":
            out[k] = torch.cat([v, torch.from_numpy(tris).cuda()])
        elif k == "positions":
            out[k] = torch.cat([v, torch.from_numpy(verts).cuda()])
        else:
            pad = torch.zeros((4 * n,) + tuple(v.shape[1:]), dtype=v.dtype,
                              device=v.device)
            out[k] = torch.cat([v, pad])
    return {k: v.contiguous() for k, v in out.items()}


def timed(fn, calls=CALLS, before=None):
    """Median ms of `calls` event-timed calls after one warm-up; `before`
    restores the inputs outside the timed span."""
    ts = []
    for i in range(calls + 1):
        if before:
            before()
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def bits_for(n):
    return max(0, int(n - 1).bit_length())


class Legs:
    def __init__(self, mesh):
        self.mesh = mesh
        self.p, self.t = mesh["positions"], mesh["indices"]
        self.v, self.m = self.p.shape[0], self.t.shape[0]
        self.L = _lib.lib()
        self.args = (_lib.ptr(self.p), self.v, _lib.F32, _lib.ptr(self.t),
                     self.m, _lib.I32)
        self.index_args = (_lib.ptr(self.t), self.m, _lib.I32, self.v)

    # -- sort -------------------------------------------------------------------
    def sort(self, torch_side):
        keys0 = self.t.reshape(-1).clone()
        vals0 = torch.arange(3 * self.m, dtype=torch.int32, device="cuda")
        keys, vals = keys0.clone(), vals0.clone()
        bits = bits_for(self.v)

        def restore():
            keys.copy_(keys0)
            vals.copy_(vals0)

        def ours():
            _lib.check(self.L.o3dmi_sort_pairs_u32(
                _lib.ptr(keys), _lib.ptr(vals), 3 * self.m, bits, stream()),
                "sort_pairs")

        res = {"pairs": 3 * self.m, "key_bits": bits}
        res["ms"], _ = timed(ours, before=restore)
        if torch_side:
            res["torch_sort_stable_ms"], _ = timed(
                lambda: torch.sort(keys0, stable=True))
            order = torch.sort(keys0, stable=True)[1]
            restore()
            ours()
            res["same_order_as_torch"] = bool((vals.long() == order).all())
        return res

    # -- vertex normals ---------------------------------------------------------
    def vertex_normals(self, torch_side):
        tn = torch.empty((self.m, 3), dtype=torch.float32, device="cuda")
        vn = torch.empty((self.v, 3), dtype=torch.float32, device="cuda")

        def ours():
            _lib.check(self.L.o3dmi_trianglemesh_vertex_normals(
                *self.args, _lib.ptr(tn), _lib.ptr(vn), 0, stream()),
                "vertex_normals")

        res = {}
        res["ms"], _ = timed(ours)
        if torch_side:
            t = self.t.long()

            def restated():
                a, b, c = self.p[t[:, 0]], self.p[t[:, 1]], self.p[t[:, 2]]
                n = torch.cross(b - a, c - a, dim=1)
                out = torch.zeros_like(self.p)
                for k in range(3):
                    out.index_add_(0, t[:, k], n)
                return out

            res["torch_index_add_ms"], _ = timed(restated)
            ours()
            ref = restated()
            scale = ref.abs().max().item()
            res["max_abs_diff_to_torch_over_scale"] = \
                (vn - ref).abs().max().item() / scale
        return res

    # -- edge table -------------------------------------------------------------
    def edge_table(self, torch_side):
        n = C.c_int64(0)

        def ours():
            _lib.check(self.L.o3dmi_trianglemesh_get_non_manifold_edges(
                *self.index_args, 1, None, -1, C.byref(n), stream()),
                "get_non_manifold_edges")

        res = {}
        res["ms"], _ = timed(ours)
        res["non_manifold_edges"] = n.value
        ours_boundary = C.c_int64(0)
        _lib.check(self.L.o3dmi_trianglemesh_get_non_manifold_edges(
            *self.index_args, 0, None, -1, C.byref(ours_boundary), stream()),
            "get_non_manifold_edges")
        res["edges_not_shared_by_two"] = ours_boundary.value
        return res

    # -- clustering -------------------------------------------------------------
    def _cluster(self):
        labels = torch.empty(self.m, dtype=torch.int32, device="cuda")
        counts = torch.empty(self.m, dtype=torch.int64, device="cuda")
        areas = torch.empty(self.m, dtype=torch.float64, device="cuda")
        n = C.c_int64(0)

        def ours():
            _lib.check(
                self.L.o3dmi_trianglemesh_cluster_connected_triangles(
                    *self.args, _lib.ptr(labels), C.byref(n),
                    _lib.ptr(counts), _lib.ptr(areas), self.m, stream()),
                "cluster_connected_triangles")
        return ours, labels, counts, areas, n

    def cluster(self, torch_side):
        ours, labels, counts, areas, n = self._cluster()
        res = {}
        res["ms"], _ = timed(ours)
        c = counts[:n.value]
        res.update(clusters=n.value, largest=int(c.max()),
                   clusters_above_100=int((c > 100).sum()),
                   area_total=float(areas[:n.value].sum()),
                   surface_area=tm.get_surface_area(self.mesh))
        return res

    # -- selection --------------------------------------------------------------
    def select(self, torch_side):
        ours, labels, counts, _, n = self._cluster()
        ours()
        keep = (counts[:n.value] > 100)[labels.long()].contiguous()
        out = {}

        def run():
            out["mesh"] = tm.select_faces_by_mask(self.mesh, keep)

        res = {}
        res["ms"], _ = timed(run)
        res.update(triangles_kept=int(out["mesh"]["indices"].shape[0]),
                   vertices_kept=int(out["mesh"]["positions"].shape[0]),
                   attributes=sorted(self.mesh))
        return res


def build_case(name):
    cfg = CASES[name]
    mesh = with_floating_components(
        room_mesh(cfg["voxel"], cfg["frames"], cfg["block_count"]),
        N_FLOATING, cfg["voxel"])
    return cfg, mesh


def case(name):
    cfg, mesh = build_case(name)
    legs = Legs(mesh)
    res = dict(cfg, vertices=legs.v, triangles=legs.m,
               floating_components=N_FLOATING)
    for leg in LEGS:
        res[leg] = getattr(legs, leg)(True)
    return res


def leg(case_name, leg_name):
    """One leg for a kernel-trace run of its own; prints one JSON line."""
    _, mesh = build_case(case_name)
    legs = Legs(mesh)
    torch.cuda.synchronize()
    res = getattr(legs, leg_name)(False)
    print(json.dumps(dict(case=case_name, leg=leg_name, calls=CALLS + 1,
                          triangles=legs.m, ms=res["ms"])))


OURS = ("Pair", "Triangle", "Corner", "VertexNormal", "SlotKeys", "NonManifold",
        "EmitEdges", "EdgeUnion", "Flatten", "Cluster", "LabelPairs",
        "RunSum", "Iota", "WidenCounts", "MaskToFlags", "FlagsToMask", "Mark",
        "TrianglesOfVertices", "Remap", "Normalize", "Scan", "Prefix",
        "Select", "Compact")


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


def short(name):
    for cut in ("(anonymous namespace)::", "o3dmi::", "void "):
        name = name.replace(cut, "")
    return name.split("(")[0].strip()


def merge(d, out_path):
    """Per leg: the library's kernels of the LAST call of the traced run (the
    launches after the mesh was built, divided evenly over the calls)."""
    with open(out_path) as f:
        res = json.load(f)
    trace = {}
    for case_name in CASES:
        for leg_name in LEGS:
            sub = os.path.join(d, "%s_%s" % (case_name, leg_name))
            if not os.path.exists(sub + ".json"):
                continue
            with open(sub + ".json") as f:
                info = json.loads(f.read().strip().splitlines()[-1])
            rows = [(short(k), ns) for k, ns in kernel_rows(sub)]
            per = {}
            for k, ns in rows:
                if k.startswith("Mesh") or not any(tag in k for tag in OURS):
                    continue  # Mesh*: the extraction that built the input
                e = per.setdefault(k, [0, 0])
                e[0] += 1
                e[1] += ns
            trace.setdefault(case_name, {})[leg_name] = dict(
                wall_ms_under_trace=info["ms"], calls=info["calls"],
                note="launch counts and kernel time of the whole traced "
                     "process (mesh set-up included) per kernel name",
                kernels={k: dict(launches=c, total_us=ns / 1e3,
                                 avg_us=ns / 1e3 / c)
                         for k, (c, ns) in sorted(per.items())})
    res["kernel_trace"] = trace
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: sorted(v) for k, v in trace.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "trianglemesh_bench.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--merge", help="directory of the per-leg trace runs")
    a = ap.parse_args()
    if a.leg:
        return leg(a.case or "200k", a.leg)
    if a.merge:
        return merge(a.merge, a.out)
    names = [a.case] if a.case else list(CASES)
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32/int32",
               calls=CALLS, timing="median of event-timed calls, ms",
               cases={n: case(n) for n in names})
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
