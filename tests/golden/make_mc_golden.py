"""Writes tests/golden/mc_reference_topology.npz: what the CPU table tests
compare the generated marching-cubes table (tools/gen_mc_tables.py) with.

Only data DERIVED from the reference's tables is stored, never the tables:
per case, the mask of edges with a vertex (edge_table), the triangle count,
and the set of directed boundary edges of its triangles in output order
(ExtractTriangleMesh writes triangle_ptr[2 - vertex], VoxelBlockGridImpl.h:
1770-1772, so every reference triangle is reversed first). A boundary edge
(a, b) is a directed triangle edge whose reverse (b, a) is no triangle edge
of the case.

    python tests/golden/make_mc_golden.py [path/to/GeometryMacros.h]
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mc_reference_topology.npz")
DEFAULT = ("/root/reference/cpp/open3d/t/geometry/kernel/GeometryMacros.h")


def _array(txt, name):
    m = re.search(r"\b%s\s*(\[[^\]]*\])+\s*=\s*\{" % name, txt)
    if m is None:
        raise ValueError("%s not found" % name)
    i, depth = m.end() - 1, 0
    for j in range(i, len(txt)):
        depth += {"{": 1, "}": -1}.get(txt[j], 0)
        if depth == 0:
            body = txt[i:j + 1]
            break
    return [int(v, 0) for v in re.findall(r"-?0x[0-9a-fA-F]+|-?\d+", body)]


def boundary_edges(tris):
    """Directed boundary edges of a triangle list, as a sorted (k, 2) array."""
    directed = set()
    for t in tris:
        for k in range(3):
            directed.add((int(t[k]), int(t[(k + 1) % 3])))
    b = sorted(e for e in directed if (e[1], e[0]) not in directed)
    return np.array(b, np.int32).reshape(-1, 2)


def derive(header=DEFAULT):
    """-> dict(edge_mask {256}, tri_count {256}, boundary {K,3} rows
    (case, from_edge, to_edge)) from the reference's GeometryMacros.h."""
    txt = open(header).read()
    edge = np.array(_array(txt, "edge_table"), np.int32)
    tri = np.array(_array(txt, "tri_table"), np.int32).reshape(256, 16)
    cnt = np.array(_array(txt, "tri_count"), np.int32)
    assert edge.shape == (256,) and cnt.shape == (256,)
    rows = []
    for case in range(256):
        t = tri[case]
        t = t[:np.argmax(t < 0)] if (t < 0).any() else t
        tris = t.reshape(-1, 3)[:, ::-1]  # output order
        for a, b in boundary_edges(tris):
            rows.append((case, a, b))
    return {"edge_mask": edge, "tri_count": cnt,
            "boundary": np.array(rows, np.int32).reshape(-1, 3)}


if __name__ == "__main__":
    d = derive(sys.argv[1] if len(sys.argv) > 1 else DEFAULT)
    np.savez(OUT, **d)
    print("wrote", OUT, {k: v.shape for k, v in d.items()})
