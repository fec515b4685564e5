"""Generates open3d_amd/csrc/mc_tables.h, the marching-cubes tables of
VoxelBlockGrid::ExtractTriangleMesh, from the cube's topology alone.

    python tools/gen_mc_tables.py            # rewrites the header
    python tools/gen_mc_tables.py --check    # exit 1 if the header is stale

Numbering. Corner i of the cube at voxel (x, y, z) is the voxel
(x, y, z) + CORNERS[i]; edge j joins corners EDGES[j] and is owned by the
voxel at its lower corner, along one axis (EDGE_OWNER). A corner is
"negative" when tsdf < 0; case = sum of 1 << i over the negative corners.

Topology. Every face of the cube contributes boundary segments:
  * a face with two sign changes gets one segment joining its two crossing
    edges;
  * a face whose two negative corners lie on a diagonal (four sign changes)
    gets two segments, each cutting off one negative corner.
Each crossing edge lies on exactly two faces, so the segments chain into
closed loops; each loop is one polygon of the surface patch in the cube.

Orientation. Each segment is directed so that, seen from the side the
TSDF gradient points to (towards the positive corners), the patch lies to
its left: the right-hand normal of every output triangle points towards
the positive side.

Triangulation. Each loop is cut into a fan from its lowest edge id, in the
loop's direction; loops are emitted by ascending lowest edge id.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "open3d_amd", "csrc", "mc_tables.h")

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0),
           (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7),
         (0, 4), (1, 5), (2, 6), (3, 7)]


def edge_owner(j):
    """(dx, dy, dz, axis): the owning voxel's offset and the edge's axis."""
    a, b = (np.array(CORNERS[k]) for k in EDGES[j])
    lo = np.minimum(a, b)
    axis = int(np.argmax(np.abs(b - a)))
    return (int(lo[0]), int(lo[1]), int(lo[2]), axis)


EDGE_OWNER = [edge_owner(j) for j in range(12)]


def faces():
    """The 6 faces as (outward normal, 4 corners in cyclic order)."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [i for i, c in enumerate(CORNERS) if c[axis] == side]
            u, v = [k for k in range(3) if k != axis]
            # cyclic order around the face
            ring = sorted(cs, key=lambda i: np.arctan2(CORNERS[i][v] - 0.5,
                                                       CORNERS[i][u] - 0.5))
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            out.append((n, ring))
    return out


FACES = faces()
EDGE_OF = {frozenset(e): j for j, e in enumerate(EDGES)}


def _mid(j):
    a, b = EDGES[j]
    return (np.array(CORNERS[a], float) + np.array(CORNERS[b], float)) / 2


def segments(case):
    """Directed segments (edge_from, edge_to) of one case."""
    neg = [(case >> i) & 1 for i in range(8)]
    segs = []
    for n, ring in FACES:
        crossing = []
        for k in range(4):
            a, b = ring[k], ring[(k + 1) % 4]
            if neg[a] != neg[b]:
                crossing.append(EDGE_OF[frozenset((a, b))])
        if not crossing:
            continue
        pieces = []  # (edge, edge, negative corners on the cut-off side)
        if len(crossing) == 2:
            cn = [c for c in ring if neg[c]]
            pieces.append((crossing[0], crossing[1], cn))
        else:
            for k in range(4):
                c = ring[k]
                if not neg[c]:
                    continue
                e1 = EDGE_OF[frozenset((c, ring[(k + 1) % 4]))]
                e2 = EDGE_OF[frozenset((c, ring[(k - 1) % 4]))]
                pieces.append((e1, e2, [c]))
        centre = np.mean([CORNERS[c] for c in ring], axis=0)
        for e1, e2, cn in pieces:
            p1, p2 = _mid(e1), _mid(e2)
            # g: in-plane direction from the negative side of the segment
            # to the positive side
            mid = (p1 + p2) / 2
            g = mid - np.mean([CORNERS[c] for c in cn], axis=0)
            if len(crossing) == 2:
                cp = [c for c in ring if not neg[c]]
                g = np.mean([CORNERS[c] for c in cp], axis=0) - \
                    np.mean([CORNERS[c] for c in cn], axis=0)
            else:
                g = centre - np.array(CORNERS[cn[0]], float)
            d = p2 - p1
            # the patch (inside the cube, direction -n) lies left of d when
            # looking down the normal g: (g x d) . n < 0
            if np.dot(np.cross(g, d), n) < 0:
                segs.append((e1, e2))
            else:
                segs.append((e2, e1))
    return segs


def loops(case):
    nxt = {}
    for a, b in segments(case):
        assert a not in nxt, (case, a)
        nxt[a] = b
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        out.append(loop)
    return out


def triangles(case):
    tris = []
    for loop in sorted(loops(case), key=min):
        k = loop.index(min(loop))
        loop = loop[k:] + loop[:k]
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def tables():
    """-> (edge_table {256} int, tri_table {256,16} int8 (-1 padded),
    tri_count {256} int)."""
    edge = np.zeros(256, np.int32)
    tri = np.full((256, 16), -1, np.int8)
    cnt = np.zeros(256, np.int32)
    for case in range(256):
        neg = [(case >> i) & 1 for i in range(8)]
        for j, (a, b) in enumerate(EDGES):
            if neg[a] != neg[b]:
                edge[case] |= 1 << j
        t = triangles(case)
        assert len(t) <= 5
        cnt[case] = len(t)
        for i, tr in enumerate(t):
            tri[case, 3 * i:3 * i + 3] = tr
    return edge, tri, cnt


def render():
    edge, tri, cnt = tables()
    L = ["// Generated by tools/gen_mc_tables.py from the cube's topology; do "
         "not edit.",
         "// Marching-cubes tables of VoxelBlockGrid::ExtractTriangleMesh "
         "(see the",
         "// generator for the numbering, the face rule and the "
         "triangulation).",
         "#pragma once", "", "namespace o3dmi {", "namespace mc {", "",
         "// corner i of the cube at voxel v is the voxel v + kCorner[i]",
         "__device__ __constant__ const signed char kCorner[8][3] = {"]
    L.append("    " + ", ".join("{%d, %d, %d}" % c for c in CORNERS) + "};")
    L.append("// edge j: owning voxel v + (dx, dy, dz), axis")
    L.append("__device__ __constant__ const signed char kEdgeOwner[12][4] = {")
    for j in range(0, 12, 4):
        L.append("    " + ", ".join("{%d, %d, %d, %d}" % EDGE_OWNER[k]
                                    for k in range(j, j + 4)) + ",")
    L.append("};")
    L.append("// bit j: edge j has a sign change")
    L.append("__device__ __constant__ const unsigned short kEdgeTable[256] = {")
    for i in range(0, 256, 8):
        L.append("    " + ", ".join("0x%03x" % v for v in edge[i:i + 8]) + ",")
    L.append("};")
    L.append("__device__ __constant__ const unsigned char kTriCount[256] = {")
    for i in range(0, 256, 16):
        L.append("    " + ", ".join("%d" % v for v in cnt[i:i + 16]) + ",")
    L.append("};")
    L.append("// triangles in output order (right-hand normal towards tsdf > 0),"
             " -1 padded")
    L.append("__device__ __constant__ const signed char kTriTable[256][16] = {")
    for i in range(256):
        L.append("    {" + ", ".join("%d" % v for v in tri[i]) + "},")
    L.append("};")
    L += ["", "}  // namespace mc", "}  // namespace o3dmi", ""]
    return "\n".join(L)


if __name__ == "__main__":
    txt = render()
    if "--check" in sys.argv:
        cur = open(HEADER).read() if os.path.exists(HEADER) else ""
        sys.exit(0 if cur == txt else 1)
    with open(HEADER, "w") as f:
        f.write(txt)
    print("wrote", HEADER)
