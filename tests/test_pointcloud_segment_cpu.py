"""CPU checks of the ClusterDBSCAN / SegmentPlane oracle
(tests/_pointcloud_segment_oracle.py) against the hand-derived golden vectors
and against itself, and of the library's pure sample function
o3dmi_plane_sample against the oracle's. No GPU."""
import ctypes as C

import numpy as np
import pytest

import _pointcloud_segment_oracle as orc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from open3d_amd import _lib
    return _lib.lib()


# ---- the oracle against the golden vectors ---------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dbscan_oracle_matches_hand_derived_labels(dtype):
    cases = orc.reference_vectors()["dbscan"]
    assert len(cases) >= 5
    for case in cases:
        pts = np.array(case["points"], dtype)
        assert orc.min_gap_ulps(pts, case["eps"]) > 4, case["name"]
        got = orc.cluster_dbscan(pts, case["eps"], case["min_points"])
        assert got.tolist() == case["labels"], case["name"]
        assert got.min() >= -1


@pytest.mark.parametrize("ransac_n", [3, 4])
@pytest.mark.parametrize("probability", [0.99999999, 1.0])
def test_segment_oracle_known_plane(ransac_n, probability):
    v = orc.reference_vectors()["segment_plane"]
    pts = np.array(v["points"])
    got = orc.segment_plane(pts, v["distance_threshold"], ransac_n, 10,
                            probability, seed=0)
    assert got["inliers"].tolist() == v["expected_inliers"]
    # x + y + z + 1 = 0, up to sign
    want = np.ones(4) / np.sqrt(3.0)
    plane = got["plane"] * np.sign(got["plane"][0])
    assert np.abs(plane - want).max() < 1e-12
    assert got["fitness"] == 1.0 and got["iterations_counted"] == 1
    assert got["final_break_iteration"] == 0


def test_plane_fits_agree_on_a_triangle():
    """Both fits give the same plane (up to sign) through three points."""
    rng = np.random.RandomState(0)
    for _ in range(20):
        p = rng.normal(size=(3, 3))
        a = orc.triangle_plane(p[0], p[1], p[2])
        b = orc.plane_from_points(p)
        assert min(np.abs(a - b).max(), np.abs(a + b).max()) < 1e-9
    line = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]])
    assert not orc.triangle_plane(*line).any()
    assert not orc.plane_from_points(np.vstack([line, 3 * line[1:2]])).any()


def test_break_iteration_rule():
    assert orc.break_iteration(1.0, 3, 0.99, 100) == 0
    assert orc.break_iteration(0.5, 3, 1.0, 100) == 100      # log(0) = -inf
    assert orc.break_iteration(1e-9, 8, 0.99, 100) == 100    # denominator 0
    assert orc.break_iteration(0.5, 3, 0.99, 100) == int(
        np.log(0.01) / np.log(1 - 0.125))
    assert orc.break_iteration(0.01, 3, 0.99, 100) == 100    # clamped


# ---- o3dmi_plane_sample against the oracle's sample function ---------------------
@pytest.mark.parametrize("ransac_n", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("n", [3, 4, 8, 1000, 2 ** 31 - 1])
def test_plane_sample_matches_oracle(lib, ransac_n, n):
    if n < ransac_n:
        out = (C.c_int64 * 8)(*[-7] * 8)
        lib.o3dmi_plane_sample(1, 0, ransac_n, n, out)
        assert list(out) == [-7] * 8  # outside the domain: nothing written
        return
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        for it in (0, 1, 63, 1000, 2 ** 40):
            out = (C.c_int64 * 8)(*[-7] * 8)
            lib.o3dmi_plane_sample(seed, it, ransac_n, n, out)
            got = list(out)[:ransac_n]
            assert got == orc.plane_sample(seed, it, ransac_n, n), (seed, it)
            assert len(set(got)) == ransac_n
            assert min(got) >= 0 and max(got) < n
            assert list(out)[ransac_n:] == [-7] * (8 - ransac_n)
            if n == ransac_n:
                assert sorted(got) == list(range(n))


def test_plane_sample_is_uniform_enough():
    """Every point of a small cloud is drawn about equally often, in every
    draw position (exact sampling without replacement)."""
    n, k, iters = 7, 4, 7000
    hits = np.zeros((k, n))
    for it in range(iters):
        for pos, v in enumerate(orc.plane_sample(5, it, k, n)):
            hits[pos, v] += 1
    # binomial(7000, 1/7): sigma = 29.3; 6 sigma
    assert np.abs(hits - iters / n).max() < 6 * np.sqrt(iters / n * (1 - 1 / n))


# ---- oracle self-checks -----------------------------------------------------------
def _blobs(n, seed, dtype):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-2, 2, size=(6, 3))
    pts = centres[rng.randint(0, 6, n)] + rng.normal(scale=0.08, size=(n, 3))
    pts[: n // 10] = rng.uniform(-3, 3, size=(n // 10, 3))
    return pts.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dbscan_labels_do_not_depend_on_worklist_order(dtype):
    pts = _blobs(600, 1, dtype)
    nbs = orc.neighbour_sets(pts, 0.12)
    for min_points in (1, 4, 10):
        a = orc.cluster_dbscan(pts, 0.12, min_points, "stack", nbs)
        b = orc.cluster_dbscan(pts, 0.12, min_points, "queue", nbs)
        assert np.array_equal(a, b)
        assert a.max() >= 1 and (min_points == 1 or (a == -1).any())


def test_dbscan_oracle_is_components_of_core_points():
    """The stated semantics, computed another way: components of the core
    graph numbered by lowest core index, borders the smallest label."""
    pts = _blobs(500, 2, np.float32)
    eps, min_points = 0.12, 5
    nbs = orc.neighbour_sets(pts, eps)
    core = np.array([len(x) >= min_points for x in nbs])
    comp = np.full(len(pts), -1)
    for i in np.nonzero(core)[0]:
        if comp[i] >= 0:
            continue
        comp[i] = i
        todo = [i]
        while todo:
            a = todo.pop()
            for j in nbs[a]:
                if core[j] and comp[j] < 0:
                    comp[j] = i
                    todo.append(j)
    roots = sorted(set(comp[core].tolist()))
    number = {r: k for k, r in enumerate(roots)}
    want = np.full(len(pts), -1, np.int32)
    for i in range(len(pts)):
        if core[i]:
            want[i] = number[comp[i]]
        else:
            near = [number[comp[j]] for j in nbs[i] if core[j]]
            want[i] = min(near) if near else -1
    assert np.array_equal(orc.cluster_dbscan(pts, eps, min_points, nbs=nbs),
                          want)


def test_segment_walk_does_not_depend_on_batch_size():
    rng = np.random.RandomState(3)
    n = 400
    pts = rng.uniform(-1, 1, size=(n, 3))
    pts[:240, 2] = 0.3 * pts[:240, 0] + rng.normal(scale=0.003, size=240)
    pts = pts.astype(np.float32)
    want = orc.segment_plane(pts, 0.01, 3, 300, 0.999, seed=7)
    assert 0 < want["iterations_counted"] < 300  # the break rule acted
    for batch in (1, 7, 64, 299):
        got = orc.segment_plane(pts, 0.01, 3, 300, 0.999, seed=7, batch=batch)
        for key in ("best_iteration", "iterations_counted",
                    "final_break_iteration", "fitness", "inlier_rmse"):
            assert got[key] == want[key], (batch, key)
        assert np.array_equal(got["inliers"], want["inliers"])
        assert np.array_equal(got["plane"], want["plane"])


def test_plane_score_tree_is_what_the_header_states():
    """Index order inside a tile, tile order across tiles."""
    rng = np.random.RandomState(4)
    pts = rng.normal(size=(1300, 3))
    plane = np.array([0.0, 0.0, 1.0, 0.0])
    counts, sums = orc.plane_score(pts, plane, 0.5)
    d = np.abs(pts[:, 2])
    total = 0.0
    for s in range(0, 1300, orc.PLANE_TILE):
        tile = 0.0
        for v in d[s:s + orc.PLANE_TILE]:
            if v < 0.5:
                tile += v * v
        total += tile
    assert counts[0] == (d < 0.5).sum() and sums[0] == total
