"""TriangleMesh ClipPlane / SlicePlane on one MI355X ->
profiles/trianglemesh_clip_bench.json.

    python tools/bench_trianglemesh_clip.py [--levels 9] [--out ...json]

Input: the unit tetrahedron subdivided `levels` times by subdivide_loop (9: a
closed mesh of 2^20 triangles and 2^19 + 2 vertices), Float32 positions, Int32
indices; with attributes, its vertex normals and random colours too. The plane
goes through the centroid of the vertices with a generic normal; slice takes
K = 1 (the contour 0) and K = 8 (contours spread over the mesh's range). Warm,
the median of 10 event-timed calls, every call with its range and finiteness
checks, its pool allocations and its waits:
  * count: the count call alone (capacity < 0: the signed values, the
           classification and the numbering of the crossing slots),
  * fill:  the call into outputs of the counted size, every optional output
           given (the index side again, then the emit),
each without and with normals and colours. Beside every time: the call's
unavoidable traffic, the inputs read once and the outputs written once (the
count call writes nothing), and that traffic over the time: how far the whole
call is from one streaming pass, no share of peak.
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
import bench_trianglemesh_subdivide as bs  # noqa: E402
from open3d_amd import _lib  # noqa: E402
from open3d_amd.core import TORCH_TO_O3DMI, stream  # noqa: E402

NORMAL = (0.3, -0.5, 0.8)


def legs(mesh, point, values, attrs):
    """-> (count leg, fill leg, sizes); values None: clip."""
    p, t = mesh["positions"], mesh["indices"]
    n = mesh["normals"] if attrs else None
    c = mesh["colors"] if attrs else None
    code = TORCH_TO_O3DMI[p.dtype]
    head = (_lib.ptr(p), p.shape[0], code, _lib.ptr(n), _lib.ptr(c), code,
            _lib.ptr(t), t.shape[0], TORCH_TO_O3DMI[t.dtype],
            (C.c_double * 3)(*point), (C.c_double * 3)(*NORMAL))
    if values is None:
        what, cell = "clip_plane", 3
        call = _lib.lib().o3dmi_trianglemesh_clip_plane
    else:
        what, cell = "slice_plane", 2
        call = _lib.lib().o3dmi_trianglemesh_slice_plane
        head += ((C.c_double * len(values))(*values), len(values))
    n_rows, n_cells = C.c_int64(0), C.c_int64(0)
    tail = (C.byref(n_rows), C.byref(n_cells), stream())
    extra = (None,) * (3 if values is None else 4)

    def count():
        _lib.check(call(*head, None, None, None, -1, None, 0, *extra, *tail),
                   what)

    count()
    rows, cells = n_rows.value, n_cells.value
    outs = [torch.empty((rows, 3), dtype=p.dtype, device="cuda")
            if a is not None else None for a in (p, n, c)]
    cell_out = torch.empty((cells, cell), dtype=t.dtype, device="cuda")
    cell_src = torch.empty(cells, dtype=t.dtype, device="cuda")
    contour = torch.empty(cells, dtype=torch.int32, device="cuda")
    row_src = torch.empty((rows, 2), dtype=t.dtype, device="cuda")
    row_t = torch.empty(rows, dtype=torch.float64, device="cuda")
    optional = [cell_src, row_src, row_t] if values is None else \
        [cell_src, contour, row_src, row_t]

    def fill():
        _lib.check(call(*head, *[_lib.ptr(o) for o in outs], rows,
                        _lib.ptr(cell_out), cells,
                        *[_lib.ptr(o) for o in optional], *tail), what)

    k = 3 if attrs else 1
    read = k * 3 * p.element_size() * p.shape[0] + \
        3 * t.element_size() * t.shape[0]
    written = sum(o.numel() * o.element_size()
                  for o in outs + [cell_out] + optional if o is not None)
    sizes = dict(rows_out=rows, cells_out=cells, count_bytes=read,
                 fill_bytes=read + written)
    return count, fill, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "trianglemesh_clip_bench.json"))
    a = ap.parse_args()
    mesh = bs.tetrahedron_subdivided(a.levels)
    p64 = mesh["positions"].to(torch.float64)
    point = p64.mean(dim=0).tolist()
    s = ((p64 - p64.mean(dim=0)) *
         torch.tensor(NORMAL, dtype=torch.float64, device="cuda")).sum(dim=1)
    lo, hi = float(s.min()), float(s.max())
    eight = [lo + (hi - lo) * (i + 0.5) / 8 for i in range(8)]
    res = dict(device=torch.cuda.get_device_name(0), dtype="float32/int32",
               calls=bt.CALLS, timing="median of event-timed calls, ms",
               input="unit tetrahedron, subdivide_loop x%d" % a.levels,
               vertices=int(mesh["positions"].shape[0]),
               triangles=int(mesh["indices"].shape[0]),
               point=point, normal=list(NORMAL), contours_k8=eight,
               traffic="inputs read once + outputs written once, bytes",
               kernel_trace="none taken", legs={})
    for which, values in (("clip", None), ("slice_k1", [0.0]),
                          ("slice_k8", eight)):
        for attrs in (False, True):
            count, fill, sizes = legs(mesh, point, values, attrs)
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
