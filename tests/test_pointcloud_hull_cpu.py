"""CPU checks of ComputeConvexHull / HiddenPointRemoval: the numpy oracle
(tests/_pointcloud_hull_oracle.py) against the goldens recorded from Qhull
(tests/golden/convex_hull, tools/make_convex_hull_goldens.py), hand cases, the
refusals, and the places the rules are written down."""
import glob
import itertools
import os
import re
import sys

import numpy as np
import pytest

import _pointcloud_hull_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "convex_hull")
GOLDENS = sorted(os.path.basename(f)[:-4]
                 for f in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def golden(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_convex_hull_goldens as tool
    finally:
        sys.path.pop(0)
    return tool


def _hull_input(g):
    """The float64 cloud whose hull the golden is (the flipped one plus the
    origin for hidden-point removal) and the point indices of its triangles."""
    P = g["points"].astype(np.float64)
    if "camera" in g:
        P = np.concatenate([orc.flip(P, g["camera"], float(g["radius"])),
                            np.zeros((1, 3))])
    return P, g["point_indices"][g["triangles"]]


def test_the_golden_set_is_complete():
    assert GOLDENS == ["cube3000_s0_f32", "cube3000_s0_f64",
                       "cube3000_s1_f32", "cube3000_s1_f64",
                       "hpr_bumpy3000_f64", "sphere1500_f32",
                       "sphere1500_f64"]
    for name in GOLDENS:
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        assert os.path.getsize(path) < 128 * 1024, name


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_equals_golden(name):
    g = golden(name)
    if "camera" in g:
        idx, tri = orc.hidden_point_removal(g["points"], g["camera"],
                                            float(g["radius"]))
    else:
        idx, tri = orc.convex_hull(g["points"])
    assert np.array_equal(idx, g["point_indices"])
    assert np.array_equal(tri, g["triangles"])


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_leaves_nothing_to_the_insertion_order(name):
    """F = 2 V - 4 and every point lies below every facet it is not a vertex
    of by at least 1e-9 E; eps is at most 2^10 * 2^-52 E = 2.3e-13 E."""
    g = golden(name)
    P, tris = _hull_input(g)
    hpr = "camera" in g
    if not hpr:
        assert len(tris) == 2 * len(g["point_indices"]) - 4
    a, b, c = P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    dist = P @ n.T - np.einsum("ij,ij->i", a, n)[None, :]
    dist[tris.T, np.arange(len(tris))[None, :]] = -np.inf
    extent = float((P.max(axis=0) - P.min(axis=0)).max())
    assert (-dist).min() >= 1e-9 * extent
    assert orc.EPS_ULPS <= 2 ** 10
    assert orc.eps_of(P) <= 2.3e-13 * extent


def test_goldens_are_fresh():
    """With scipy at hand the goldens are recorded again in memory (which
    asserts: no coplanar point, F = 2 V - 4, the margin) and compared."""
    pytest.importorskip("scipy.spatial")
    tool = _tool()
    assert sorted(tool.CASES) == GOLDENS
    for name in GOLDENS:
        fresh, g = tool.record(name), golden(name)
        assert sorted(fresh) == sorted(g), name
        for key in g:
            assert fresh[key].dtype == g[key].dtype, (name, key)
            assert np.array_equal(fresh[key], g[key]), (name, key)


# ---- hand cases ---------------------------------------------------------------------
TETRA = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
OCTA = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1],
                 [0, 0, -1]], np.float64)
CUBE = np.array(list(itertools.product([0, 1], repeat=3)), np.float64)


def six_volume(P, idx, tri):
    """Sum of a . (b x c) over the triangles, in Python integers."""
    total = 0
    for t in tri:
        a, b, c = [[int(v) for v in P[idx[k]]] for k in t]
        total += (a[0] * (b[1] * c[2] - b[2] * c[1]) +
                  a[1] * (b[2] * c[0] - b[0] * c[2]) +
                  a[2] * (b[0] * c[1] - b[1] * c[0]))
    return total


def test_tetrahedron_in_all_24_orders():
    seen = set()
    for perm in itertools.permutations(range(4)):
        perm = np.array(perm)
        idx, tri = orc.convex_hull(TETRA[perm])
        assert np.array_equal(idx, np.arange(4)) and len(tri) == 4
        # the same four triangles on the points themselves
        seen.add(tuple(sorted(tuple(sorted(perm[t])) for t in tri)))
        assert orc.edges_closed_and_oriented(tri)
        assert six_volume(TETRA[perm], idx, tri) == 1
    assert len(seen) == 1
    idx, tri = orc.convex_hull(TETRA)
    assert tri.tolist() == [[0, 1, 3], [0, 2, 1], [0, 3, 2], [1, 2, 3]]


def test_tetrahedron_plus_centroid():
    P = np.concatenate([TETRA[:2], TETRA.mean(axis=0)[None], TETRA[2:]])
    idx, tri = orc.convex_hull(P)
    assert idx.tolist() == [0, 1, 3, 4] and len(tri) == 4


def test_octahedron():
    idx, tri = orc.convex_hull(OCTA)
    assert idx.tolist() == list(range(6)) and len(tri) == 8
    assert orc.edges_closed_and_oriented(tri) and orc.euler(tri) == 2
    assert six_volume(OCTA, idx, tri) == 8


def test_cube_corners():
    idx, tri = orc.convex_hull(CUBE)
    assert idx.tolist() == list(range(8)) and len(tri) == 12
    assert orc.edges_closed_and_oriented(tri)
    assert orc.euler(tri) == 2
    assert six_volume(CUBE, idx, tri) == 6
    # canonical: lowest vertex first, rows sorted
    assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 0] < tri[:, 2]).all()
    assert tri.tolist() == sorted(tri.tolist())


def test_coincident_points_only_the_lowest_index_is_a_vertex():
    idx, tri = orc.convex_hull(np.concatenate([CUBE, CUBE]))
    single = orc.convex_hull(CUBE)
    assert np.array_equal(idx, single[0]) and np.array_equal(tri, single[1])


# ---- refusals -----------------------------------------------------------------------
def _refused(fn, *args):
    with pytest.raises(orc.HullRefused) as e:
        fn(*args)
    return e.value.status


def refusal_cases():
    """name -> (points, camera or None, radius, status): shared with the GPU
    test."""
    rng = np.random.default_rng(11)
    sphere = rng.standard_normal((50, 3))
    sphere /= np.linalg.norm(sphere, axis=1, keepdims=True)
    nan = sphere.copy()
    nan[17, 1] = np.nan
    return {
        "three_points": (TETRA[:3], None, 0, orc.INVALID_ARG),
        "coplanar": (np.concatenate([rng.random((100, 2)),
                                     np.full((100, 1), 0.5)], axis=1), None,
                     0, orc.SINGULAR),
        # multiples of 1 / 128: exact in float32 too
        "collinear": (np.outer(rng.permutation(100), [1.0, 2.0, 3.0]) / 128,
                      None, 0, orc.SINGULAR),
        "copies": (np.full((100, 3), 0.25), None, 0, orc.SINGULAR),
        "nan": (nan, None, 0, orc.INVALID_ARG),
        "radius_zero": (sphere, (0.0, 0.0, 3.0), 0.0, orc.INVALID_ARG),
        "point_at_camera": (sphere, tuple(sphere[7]), 10.0, orc.INVALID_ARG),
    }


@pytest.mark.parametrize("name", sorted(refusal_cases()))
def test_refusals(name):
    points, camera, radius, status = refusal_cases()[name]
    if camera is None:
        assert _refused(orc.convex_hull, points) == status
    else:
        assert _refused(orc.hidden_point_removal, points, camera,
                        radius) == status


# ---- where the rules are written down -----------------------------------------------
def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_abi_listing_and_constants():
    from open3d_amd import _lib
    host_h = _read("include", "o3d_mi355x_host.h")
    seam = _read("open3d_amd", "csrc", "pointcloud_hull.h")
    for name in ("o3dmi_pointcloud_convex_hull",
                 "o3dmi_pointcloud_hidden_point_removal"):
        assert name + "(" in host_h and name in _lib.PROTOTYPES, name
    stats = "o3dmi_internal_pointcloud_hull_stats"
    assert stats in seam and stats in _lib.INTERNAL_PROTOTYPES
    ulps = int(re.search(r"constexpr int kHullEpsUlps = (\d+);",
                         seam).group(1))
    assert ulps == orc.EPS_ULPS and ulps <= 2 ** 10
    assert "#define O3DMI_HULL_EPS_ULPS %d\n" % ulps in host_h
    assert "constexpr int kHullBlock = kBlock;" in seam
    for rule in ("eps |n|", "lowest point index", "O3DMI_ERR_SINGULAR",
                 "ascending input point", "counter-clockwise",
                 "sorted by (v0, v1, v2)", "coincident points",
                 "O3DMI_ERR_CAPACITY", "n >= 2^31 - 1"):
        assert rule in host_h, rule


def test_switches_and_docs_are_listed():
    switches = _read("docs", "switches.md")
    driver = _read("open3d_amd", "csrc", "host", "pointcloud_hull.cpp")
    assert "`O3DMI_HULL_WALK`" in switches and "O3DMI_HULL_WALK" in driver
    assert "ONCE PER ROUND" in driver  # the host waits, as the header says
    doc = _read("docs", "pointcloud_convex_hull.md")
    for word in ("kHullEpsUlps", "horizon", "PrefixSumAsync", "ring"):
        assert word in doc, word
    readme = _read("README.md")
    assert "pointcloud_hull.hip" in readme
    assert "host/pointcloud_hull.cpp" in readme


def test_python_layer_refuses_joggle():
    from open3d_amd import pointcloud, trianglemesh
    with pytest.raises(ValueError, match="joggle"):
        pointcloud.compute_convex_hull({}, joggle_inputs=True)
    with pytest.raises(ValueError):
        trianglemesh.compute_convex_hull({"positions": None},
                                         joggle_inputs=True)
