"""GPU tests of PointCloud::ClusterDBSCAN and PointCloud::SegmentPlane against
the numpy oracle (tests/_pointcloud_segment_oracle.py): labels, inlier lists
and the walk's counters are exact, the d^2 sums within the float64 summation
bound, the refitted plane within 1e-12.

Every generated DBSCAN cloud is first cleaned on the CPU of pairs whose d2 is
within 4 ulp of eps^2 (the later point of such a pair is dropped); every score
input is checked to have no distance within 4 ulp of the threshold."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _pointcloud_segment_oracle as orc

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 7
F32, F64 = 0, 1
DTYPES = [np.float32, np.float64]


def _pc():
    from open3d_amd import pointcloud
    return pointcloud


def _L():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- DBSCAN ---------------------------------------------------------------------
def _clean(points, eps):
    """-> (points without near-threshold pairs, their neighbour sets)."""
    pts = np.ascontiguousarray(points)
    for _ in range(4):
        near = []
        nbs = orc.neighbour_sets(pts, eps, near)
        if not near:
            return pts, nbs
        pts = np.delete(pts, sorted({j for _, j in near}), axis=0)
    raise AssertionError("pairs within 4 ulp of eps^2 remain")


def _gpu_labels(pts, eps, min_points):
    labels, clusters, noise = _pc().cluster_dbscan(
        {"positions": _dev(pts)}, eps, min_points, return_counts=True)
    assert labels.dtype == torch.int32 and labels.shape == (len(pts),)
    labels = labels.cpu().numpy()
    # the counters are the label statistics; -2 never leaves the call
    assert clusters == (int(labels.max()) + 1 if len(labels) else 0)
    assert noise == int((labels == -1).sum())
    assert len(labels) == 0 or labels.min() >= -1
    return labels


def _check(pts, eps, min_points, nbs=None):
    if nbs is None:
        pts, nbs = _clean(pts, eps)
    want = orc.cluster_dbscan(pts, eps, min_points, nbs=nbs)
    got = _gpu_labels(pts, eps, min_points)
    assert got.tobytes() == want.tobytes()
    return want


BLOB_EPS, BLOB_MIN = 0.05, 10


def _blob_points(n=20000):
    rng = np.random.RandomState(1)
    centres = rng.uniform(-1.5, 1.5, size=(8, 3))
    pts = centres[rng.randint(0, 8, n)] + rng.normal(scale=0.1, size=(n, 3))
    pts[: n // 10] = rng.uniform(-2, 2, size=(n // 10, 3))
    return pts


@functools.lru_cache(maxsize=None)
def _blobs(kind):
    """The 20 000-point cloud (more points than one pass of the grid-stride
    wave loop holds waves): cleaned points, neighbour sets, oracle labels."""
    pts = _blob_points()
    pts = {"f32": pts.astype(np.float32), "f64": pts,
           "shifted": (pts + 1000.0).astype(np.float32)}[kind]
    pts, nbs = _clean(pts, BLOB_EPS)
    assert len(pts) > 19000
    want = orc.cluster_dbscan(pts, BLOB_EPS, BLOB_MIN, nbs=nbs)
    assert want.max() >= 5 and (want == -1).sum() > 1000
    return pts, nbs, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_dbscan_small_sizes(n, dtype):
    pts = _blob_points(2000)[1000:1000 + n].astype(dtype) * 0.25
    want = _check(pts.reshape(n, 3), 0.05, 3)
    assert n < 63 or want.max() >= 0


@pytest.mark.parametrize("kind", ["f32", "f64", "shifted"])
def test_dbscan_blobs(kind):
    """shifted: the cloud moved by 1000 m in Float32 (cells are binned in
    float64 on both sides); equal to the oracle on the shifted input."""
    pts, _, want = _blobs(kind)
    got = _gpu_labels(pts, BLOB_EPS, BLOB_MIN)
    assert got.tobytes() == want.tobytes()


def test_dbscan_two_runs_same_bytes():
    pts, _, _ = _blobs("f32")
    a = _gpu_labels(pts, BLOB_EPS, BLOB_MIN)
    b = _gpu_labels(pts, BLOB_EPS, BLOB_MIN)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dbscan_reference_vectors(dtype):
    for case in orc.reference_vectors()["dbscan"]:
        pts = np.array(case["points"], dtype)
        got = _gpu_labels(pts, case["eps"], case["min_points"])
        assert got.tolist() == case["labels"], case["name"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_dbscan_shuffled_chain_is_one_cluster(dtype):
    """5000 points spaced 0.9 eps in shuffled index order: long union paths."""
    n, eps = 5000, 1.0
    x = 0.9 * eps * np.random.RandomState(2).permutation(n)
    pts = np.stack([x, np.zeros(n), np.zeros(n)], 1).astype(dtype)
    want = _check(pts, eps, 2)
    assert not want.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dbscan_bridge_keeps_two_clusters(dtype):
    """Two dense groups and one non-core point within eps of a core of each."""
    rng = np.random.RandomState(3)
    a = rng.uniform(-0.2, 0.2, size=(40, 3))
    b = rng.uniform(-0.2, 0.2, size=(40, 3)) + [3.0, 0, 0]
    a[0], b[0] = [0.6, 0, 0], [2.4, 0, 0]      # cores nearest the bridge
    bridge = np.array([[1.5, 0.0, 0.0]])       # 0.9 from each, 3 neighbours
    pts = np.vstack([b[:20], bridge, a, b[20:]]).astype(dtype)
    want = _check(pts, 1.0, 4)
    assert want.max() == 1 and want[20] == 0 and (want == -1).sum() == 0
    assert want[0] == 0 and want[21] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_dbscan_border_point_at_index_zero(dtype):
    """Index 0 borders the cluster whose lowest core index is the higher one:
    numbering follows the core indices, the early -1 is overwritten."""
    rng = np.random.RandomState(4)
    a = rng.uniform(-0.2, 0.2, size=(30, 3))
    b = rng.uniform(-0.2, 0.2, size=(30, 3)) + [5.0, 0, 0]
    b[0] = [5.6, 0, 0]
    border = np.array([[6.5, 0.0, 0.0]])       # only b[0] is within eps
    pts = np.vstack([border, a, b]).astype(dtype)
    want = _check(pts, 1.0, 4)
    assert want[0] == 1 and want[1] == 0 and want[31] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_dbscan_dense_ball_and_duplicates(dtype):
    """300 points in one eps-ball (several 64-candidate batches per wave),
    with exact duplicates among them."""
    rng = np.random.RandomState(5)
    pts = rng.uniform(-0.2, 0.2, size=(300, 3))
    pts[100:150] = pts[0]
    pts[150:160] = pts[1]
    far = rng.uniform(-0.2, 0.2, size=(5, 3)) + [4.0, 0, 0]
    pts = np.vstack([far[:2], pts, far[2:]]).astype(dtype)
    want = _check(pts, 1.0, 6)
    assert want.max() == 0 and (want == -1).sum() == 5


@pytest.mark.parametrize("dtype", DTYPES)
def test_dbscan_min_points_edges(dtype):
    pts, nbs = _clean(_blob_points(1500).astype(dtype), 0.08)
    n = len(pts)
    for min_points in (0, 1):
        want = _check(pts, 0.08, min_points, nbs)
        assert want.min() >= 0          # every point is core
    want = _check(pts, 0.08, n + 1, nbs)
    assert (want == -1).all()
    want = _check(pts, 0.08, n, nbs)
    assert (want == -1).all()


def _dbscan_raw(pts_t, n, dtype, eps, min_points, labels_t):
    L = _L()
    clusters, noise = C.c_int64(-7), C.c_int64(-7)
    st = L.lib().o3dmi_pointcloud_cluster_dbscan(
        L.ptr(pts_t), n, dtype, C.c_double(eps), min_points, L.ptr(labels_t),
        C.byref(clusters), C.byref(noise), None)
    torch.cuda.synchronize()
    return st, clusters.value, noise.value


def test_dbscan_errors_leave_the_labels_untouched():
    n = 100
    pts = np.random.RandomState(6).rand(n, 3).astype(np.float32)
    bad = pts.copy()
    bad[17, 1] = np.nan
    inf = pts.copy()
    inf[99, 2] = np.inf
    labels = torch.full((n,), -123, dtype=torch.int32, device="cuda")
    table = [(pts, 0.0, 3), (pts, -1.0, 3), (pts, float("nan"), 3),
             (pts, 0.1, -1), (bad, 0.1, 3), (inf, 0.1, 3)]
    for p, eps, min_points in table:
        p_dev = _dev(p)
        st, clusters, noise = _dbscan_raw(p_dev, n, F32, eps, min_points,
                                          labels)
        assert st == INVALID_ARG, (eps, min_points)
        assert (clusters, noise) == (-7, -7)
        assert bool((labels == -123).all())
    L = _L()
    pts_dev = _dev(pts)
    for points, out in ((None, labels), (pts_dev, None)):
        st = L.lib().o3dmi_pointcloud_cluster_dbscan(
            L.ptr(points), n, F32, C.c_double(0.1), 3, L.ptr(out), None, None,
            None)
        assert st == INVALID_ARG
    # n == 0 is fine, with or without buffers; the counters are optional
    st, clusters, noise = _dbscan_raw(None, 0, F32, 0.1, 3, None)
    assert (st, clusters, noise) == (0, 0, 0)
    st = L.lib().o3dmi_pointcloud_cluster_dbscan(
        L.ptr(pts_dev), n, F32, C.c_double(0.1), 3, L.ptr(labels), None,
        None, None)
    assert st == 0 and int(labels.min()) >= -1


# ---- o3dmi_plane_score ----------------------------------------------------------
SCORE_THRESHOLD = 0.1


@functools.lru_cache(maxsize=None)
def _score_inputs():
    rng = np.random.RandomState(7)
    pts = rng.uniform(-1, 1, size=(70000, 3))
    normals = rng.normal(size=(300, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    planes = np.hstack([normals, rng.uniform(-0.5, 0.5, size=(300, 1))])
    planes[0] = [0, 0, 0, 0.05]   # every point inside
    planes[1] = [0, 0, 0, 5.0]    # none
    return pts, planes


def _score(pts, planes, threshold):
    L = _L()
    b = len(planes)
    counts = torch.full((b,), -1, dtype=torch.int64, device="cuda")
    sums = torch.full((b,), -1.0, dtype=torch.float64, device="cuda")
    p, q = _dev(pts), _dev(planes)
    L.check(L.lib().o3dmi_plane_score(
        L.ptr(p), len(pts), L.F64 if pts.dtype == np.float64 else L.F32,
        L.ptr(q), b, C.c_double(threshold), L.ptr(counts), L.ptr(sums), None),
        "plane_score")
    torch.cuda.synchronize()
    return counts.cpu().numpy(), sums.cpu().numpy()


def _check_score(pts, planes):
    p64 = pts.astype(np.float64)
    dist = orc.distances(p64, planes)
    gap = np.abs(dist - SCORE_THRESHOLD)
    assert gap.min() > 4 * np.spacing(SCORE_THRESHOLD)
    want_counts, want_sums = orc.plane_score(p64, planes, SCORE_THRESHOLD)
    counts, sums = _score(pts, planes, SCORE_THRESHOLD)
    assert np.array_equal(counts, want_counts)
    # float64 summation bound: n terms, each addition within 2^-53 relative
    bound = len(pts) * 2.0 ** -52 * want_sums
    assert (np.abs(sums - want_sums) <= bound).all()
    assert counts[0] == len(pts)
    if len(planes) > 1:
        assert counts[1] == 0 and sums[1] == 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
@pytest.mark.parametrize("b", [1, 63, 64, 65, 300])
def test_plane_score_sizes(b, n):
    pts, planes = _score_inputs()
    _check_score(pts[:n].astype(np.float32), planes[:b])


def test_plane_score_float64_points():
    pts, planes = _score_inputs()
    _check_score(pts[:5000], planes[:65])


def test_plane_score_errors():
    L = _L()
    pts, planes = _score_inputs()
    p, q = _dev(pts[:10].astype(np.float32)), _dev(planes[:2])
    counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    sums = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    for n, b, thr, pp, qq in ((10, 2, 0.0, p, q), (10, 2, -1.0, p, q),
                              (-1, 2, 0.1, p, q), (10, -1, 0.1, p, q),
                              (10, 2, 0.1, None, q), (10, 2, 0.1, p, None)):
        st = L.lib().o3dmi_plane_score(L.ptr(pp), n, F32, L.ptr(qq), b,
                                       C.c_double(thr), L.ptr(counts),
                                       L.ptr(sums), None)
        assert st == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((counts == -1).all()) and bool((sums == -1.0).all())


# ---- SegmentPlane -----------------------------------------------------------------
def _segment(pts, threshold, ransac_n, iters, probability, seed):
    plane, inliers, info = _pc().segment_plane(
        {"positions": _dev(pts)}, threshold, ransac_n, iters, probability,
        seed, return_info=True)
    assert plane.dtype == torch.float64 and plane.shape == (4,)
    assert plane.is_cuda and inliers.is_cuda and inliers.dtype == torch.int64
    return plane.cpu().numpy(), inliers.cpu().numpy(), info


def _check_segment(pts, threshold, ransac_n, iters, probability, seed):
    want = orc.segment_plane(pts, threshold, ransac_n, iters, probability,
                             seed)
    plane, inliers, info = _segment(pts, threshold, ransac_n, iters,
                                    probability, seed)
    for key in ("best_iteration", "iterations_counted",
                "final_break_iteration"):
        assert info[key] == want[key], key
    assert np.array_equal(inliers, want["inliers"])
    scale = max(1.0, float(np.abs(want["plane"]).max()))
    assert np.abs(plane - want["plane"]).max() <= 1e-12 * scale
    assert abs(info["fitness"] - want["fitness"]) <= 1e-15
    assert abs(info["inlier_rmse"] - want["inlier_rmse"]) <= \
        1e-12 * max(want["inlier_rmse"], 1e-300)
    return want


def _noisy_plane(n, outliers, threshold, seed):
    """A tilted plane with noise sigma = threshold / 3 and uniform outliers."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform(-1, 1, size=(n, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.1 + rng.normal(
        scale=threshold / 3, size=n)
    pts = np.column_stack([xy, z])
    k = int(round(outliers * n))
    pts[rng.permutation(n)[:k]] = rng.uniform(-1, 1, size=(k, 3))
    return pts


@pytest.mark.parametrize("ransac_n", [3, 4])
@pytest.mark.parametrize("probability", [0.99999999, 1.0])
def test_segment_plane_known_plane(ransac_n, probability):
    v = orc.reference_vectors()["segment_plane"]
    for dtype in DTYPES:
        pts = np.array(v["points"], dtype)
        plane, inliers, info = _segment(pts, v["distance_threshold"], ransac_n,
                                        10, probability, 0)
        assert inliers.tolist() == v["expected_inliers"]
        want = np.ones(4) / np.sqrt(3.0)
        assert np.abs(plane * np.sign(plane[0]) - want).max() < 1e-12
        assert info["fitness"] == 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ransac_n", [3, 6])
@pytest.mark.parametrize("iters,probability",
                         [(1000, 0.99999999), (1000, 1.0), (3000, 1.0)])
def test_segment_plane_noisy_plane(iters, probability, ransac_n, dtype):
    """probability 1 keeps the bound at num_iterations: 3000 iterations cross
    the first batch of 1024; the default probability ends the walk early."""
    pts = _noisy_plane(5000, 0.4, 0.01, 11).astype(dtype)
    want = _check_segment(pts, 0.01, ransac_n, iters, probability, 5)
    assert want["fitness"] > 0.5
    if probability == 1.0:
        assert want["iterations_counted"] == iters
    else:
        assert want["iterations_counted"] < iters


def test_segment_plane_early_exit_on_an_exact_plane():
    rng = np.random.RandomState(12)
    pts = np.column_stack([rng.uniform(-1, 1, size=(2000, 2)),
                           np.zeros(2000)]).astype(np.float32)
    want = _check_segment(pts, 0.01, 3, 500, 0.99999999, 0)
    assert want["iterations_counted"] == 1 and want["fitness"] == 1.0
    assert want["final_break_iteration"] == 0


@pytest.mark.parametrize("seed", [1, 2])
def test_segment_plane_mostly_outliers(seed):
    pts = _noisy_plane(5000, 0.99, 0.01, 13).astype(np.float32)
    want = _check_segment(pts, 0.01, 3, 2000, 0.99999999, seed)
    assert want["iterations_counted"] == 2000 and want["best_iteration"] >= 0


def test_segment_plane_seed_changes_the_walk():
    pts = _noisy_plane(5000, 0.99, 0.01, 13).astype(np.float32)
    a = _segment(pts, 0.01, 3, 2000, 0.99999999, 1)
    b = _segment(pts, 0.01, 3, 2000, 0.99999999, 2)
    again = _segment(pts, 0.01, 3, 2000, 0.99999999, 1)
    assert a[2]["best_iteration"] != b[2]["best_iteration"]
    assert a[0].tobytes() == again[0].tobytes()
    assert a[1].tobytes() == again[1].tobytes() and a[2] == again[2]


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_segment_plane_collinear_points(ransac_n):
    t = np.arange(-20, 21, dtype=np.float64)
    pts = np.outer(t, [1.0, 2.0, 3.0]).astype(np.float32)
    plane, inliers, info = _segment(pts, 0.01, ransac_n, 50, 0.99999999, 0)
    assert not plane.any() and len(inliers) == 0
    assert info["best_iteration"] == -1 and info["iterations_counted"] == 0


def test_segment_plane_repeated_points_skip_zero_planes():
    """Three distinct points repeated: a sample with a repeat has norm 0, is
    skipped and not counted."""
    tri = np.array([[0.0, 0, 0], [1, 0, 0.5], [0, 1, -0.25]])
    pts = np.tile(tri, (30, 1)).astype(np.float64)
    seed = next(s for s in range(50) if orc.segment_plane(
        pts, 0.01, 3, 40, 0.99999999, s)["best_iteration"] >= 2)
    want = _check_segment(pts, 0.01, 3, 40, 0.99999999, seed)
    assert want["iterations_counted"] == 1 and want["fitness"] == 1.0
    assert len(want["inliers"]) == 90


def test_segment_plane_tie_keeps_the_lower_iteration():
    """Two parallel sheets of 50 points each: every sample inside one sheet
    scores fitness 0.5, rmse 0."""
    rng = np.random.RandomState(14)
    xy = rng.uniform(-1, 1, size=(50, 2))
    pts = np.vstack([np.column_stack([xy, np.zeros(50)]),
                     np.column_stack([xy, np.ones(50)])])
    pts = pts[rng.permutation(100)].astype(np.float32)
    want = _check_segment(pts, 0.01, 3, 200, 1.0, 3)
    p64 = pts.astype(np.float64)
    planes = np.array([orc.hypothesis(p64, 3, i, 3) for i in range(200)])
    counts, sums = orc.plane_score(p64, planes, 0.01)
    top = np.nonzero((counts == 50) & (sums == 0))[0]
    assert counts.max() == 50 and len(top) >= 2
    assert want["best_iteration"] == top[0]
    assert want["fitness"] == 0.5 and want["inlier_rmse"] == 0.0


def test_segment_plane_errors_write_nothing():
    L = _L()
    n = 50
    pts = _noisy_plane(n, 0.2, 0.01, 15).astype(np.float32)
    bad = pts.copy()
    bad[7, 0] = np.inf
    nan = pts.copy()
    nan[49, 2] = np.nan
    inliers = torch.full((n,), -5, dtype=torch.int64, device="cuda")

    def call(p, n_pts, thr, ransac_n, iters, prob):
        plane = (C.c_double * 4)(9.0, 9.0, 9.0, 9.0)
        m = C.c_int64(-7)
        info = L.SegmentPlaneInfoC(-9, -9, -9, -9.0, -9.0)
        p_dev = _dev(p)
        st = L.lib().o3dmi_pointcloud_segment_plane(
            L.ptr(p_dev), n_pts, F32, C.c_double(thr), ransac_n, iters,
            C.c_double(prob), 0, plane, L.ptr(inliers), C.byref(m),
            C.byref(info), None)
        torch.cuda.synchronize()
        assert list(plane) == [9.0] * 4 and m.value == -7
        assert info.best_iteration == -9 and info.fitness == -9.0
        assert bool((inliers == -5).all())
        return st

    table = [(pts, n, 0.01, 3, 10, 0.0), (pts, n, 0.01, 3, 10, -1.0),
             (pts, n, 0.01, 3, 10, 1.5), (pts, n, 0.01, 3, 10, float("nan")),
             (pts, n, 0.01, 2, 10, 0.99), (pts, 2, 0.01, 3, 10, 0.99),
             (pts, 5, 0.01, 6, 10, 0.99), (pts, n, 0.01, 3, 0, 0.99),
             (pts, n, 0.0, 3, 10, 0.99), (pts, n, -0.01, 3, 10, 0.99),
             (bad, n, 0.01, 3, 10, 0.99), (nan, n, 0.01, 3, 10, 0.99)]
    for row in table:
        assert call(*row) == INVALID_ARG, row[1:]
    assert call(pts, n, 0.01, 9, 10, 0.99) == UNSUPPORTED
