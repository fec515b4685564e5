"""TriangleMesh SubdivideMidpoint / SubdivideLoop on one MI355X ->
profiles/trianglemesh_subdivide_bench.json.

    python tools/bench_trianglemesh_subdivide.py [--levels 9] [--out ...json]

Input: the unit tetrahedron subdivided `levels` times by subdivide_loop itself
(9: a closed mesh of 2^20 triangles and 2^19 + 2 vertices), Float32 positions,
Int32 indices; with attributes, its vertex normals and random colours too.
One iteration of each call, warm, the median of 10 event-timed calls, every
call with its range and finiteness checks, its pool allocations and its waits:
  * count: the count call alone (vertex_capacity < 0: the index side),
  * fill:  the call into outputs of the counted size (the index side again,
           then the attributes),
each without and with normals and colours. Beside every time: the call's
unavoidable traffic, the inputs read once and the outputs written once (the
count call writes nothing), and that traffic over the time. The sorts of the
edge table move several times those bytes, so this rate shows how far the
sort-dominated index side is from a streaming pass; it is no share of peak.
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
from open3d_amd import _lib  # noqa: E402
from open3d_amd import trianglemesh as tm  # noqa: E402
from open3d_amd.core import TORCH_TO_O3DMI, stream  # noqa: E402

CALLS = {"midpoint": "o3dmi_trianglemesh_subdivide_midpoint",
         "loop": "o3dmi_trianglemesh_subdivide_loop"}


def tetrahedron_subdivided(levels):
    p = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]],
                     dtype=torch.float32, device="cuda")
    t = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]],
                     dtype=torch.int32, device="cuda")
    mesh = tm.subdivide_loop({"positions": p, "indices": t}, levels)
    full = tm.compute_vertex_normals(mesh)
    g = torch.Generator(device="cuda").manual_seed(0)
    return {"positions": mesh["positions"], "indices": mesh["indices"],
            "normals": full["normals"].contiguous(),
            "colors": torch.rand(mesh["positions"].shape, generator=g,
                                 device="cuda")}


def legs(mesh, which, attrs):
    """-> (count leg, fill leg, sizes) of one iteration."""
    p, t = mesh["positions"], mesh["indices"]
    n = mesh["normals"] if attrs else None
    c = mesh["colors"] if attrs else None
    call = getattr(_lib.lib(), CALLS[which])
    code = TORCH_TO_O3DMI[p.dtype]
    head = (_lib.ptr(p), p.shape[0], code, _lib.ptr(n), _lib.ptr(c), code,
            _lib.ptr(t), t.shape[0], TORCH_TO_O3DMI[t.dtype], 1)
    n_v, n_t = C.c_int64(0), C.c_int64(0)

    def count():
        _lib.check(call(*head, None, None, None, -1, None, C.byref(n_v),
                        C.byref(n_t), stream()), which)

    count()
    outs = [torch.empty((n_v.value, 3), dtype=p.dtype, device="cuda")
            if a is not None else None for a in (p, n, c)]
    tris = torch.empty((n_t.value, 3), dtype=t.dtype, device="cuda")

    def fill():
        _lib.check(call(*head, *[_lib.ptr(o) for o in outs], n_v.value,
                        _lib.ptr(tris), C.byref(n_v), C.byref(n_t), stream()),
                   which)

    k = 3 if attrs else 1
    row = 3 * p.element_size()
    tri_row = 3 * t.element_size()
    read = k * row * p.shape[0] + tri_row * t.shape[0]
    written = k * row * n_v.value + tri_row * n_t.value
    sizes = dict(vertices_out=n_v.value, triangles_out=n_t.value,
                 count_bytes=read, fill_bytes=read + written)
    return count, fill, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "trianglemesh_subdivide_bench.json"))
    a = ap.parse_args()
    mesh = tetrahedron_subdivided(a.levels)
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32/int32",
               calls=bt.CALLS, timing="median of event-timed calls, ms",
               input="unit tetrahedron, subdivide_loop x%d" % a.levels,
               vertices=int(mesh["positions"].shape[0]),
               triangles=int(mesh["indices"].shape[0]),
               traffic="inputs read once + outputs written once, bytes",
               legs={})
    for which in CALLS:
        for attrs in (False, True):
            count, fill, sizes = legs(mesh, which, attrs)
            leg = dict(sizes)
            for name, fn in (("count", count), ("fill", fill)):
                ms, all_ms = bt.timed(fn)
                leg[name + "_ms"] = ms
                leg[name + "_ms_min_max"] = [float(np.min(all_ms)),
                                             float(np.max(all_ms))]
                leg[name + "_gb_per_s"] = \
                    sizes[name + "_bytes"] / (ms * 1e-3) / 1e9
            res["legs"]["%s_%s" % (which, "attrs" if attrs else "plain")] = leg
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
