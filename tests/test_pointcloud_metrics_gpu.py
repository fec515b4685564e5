"""GPU tests of PointCloud::ComputeMetrics and the nearest-point distances
against the numpy oracle (tests/_pointcloud_metrics_oracle.py). Everything is
compared bit for bit -- distances, indices, float64 sums, maxima, counts and the
final values; the only tolerance is the one upstream's own vector carries."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _pointcloud_metrics_oracle as orc

pytestmark = pytest.mark.gpu

INVALID_ARG, CAPACITY = 1, 3
F32, F64 = 0, 1
DTYPES = [np.float32, np.float64]
CODE = {np.float32: F32, np.float64: F64}
ALL = [orc.CHAMFER, orc.HAUSDORFF, orc.FSCORE]
RADII = (0.01, 0.11, 0.15, 0.18)
POISON = -777.0


def _pc():
    from open3d_amd import pointcloud
    return pointcloud


def _L():
    from open3d_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the two ABI calls ---------------------------------------------------------------
def abi_nearest(target, queries, with_idx=True):
    """-> (status, dist {q}, idx {q} or None); the outputs start poisoned."""
    L = _L()
    dtype = queries.dtype.type
    t, p = _dev(target), _dev(queries)
    dist = torch.full((len(queries),), POISON, dtype=p.dtype, device="cuda")
    idx = torch.full((len(queries),), -9, dtype=torch.int32,
                     device="cuda") if with_idx else None
    st = L.lib().o3dmi_pointcloud_nearest_distance(
        L.ptr(t), len(target), L.ptr(p), len(queries), CODE[dtype],
        L.ptr(dist), L.ptr(idx), None)
    torch.cuda.synchronize()
    return st, dist.cpu().numpy(), idx.cpu().numpy() if with_idx else None


def abi_metrics(p1, p2, metrics=ALL, radii=RADII, capacity=None):
    """-> (status, values float32 {capacity}, raw dict); outputs start
    poisoned."""
    L = _L()
    dtype = p1.dtype.type
    a, b = _dev(p1), _dev(p2)
    r = len(radii)
    n_values = sum(r if m == orc.FSCORE else 1 for m in metrics)
    cap = n_values if capacity is None else capacity
    values = (C.c_float * max(cap, 1))(*([POISON] * max(cap, 1)))
    counts = (C.c_int64 * max(2 * r, 1))(*([-9] * max(2 * r, 1)))
    raw = L.MetricsRawC()
    raw.sum[0] = raw.sum[1] = raw.max[0] = raw.max[1] = POISON
    raw.second_pass_queries[0] = raw.second_pass_queries[1] = -9
    raw.counts = C.cast(counts, C.POINTER(C.c_int64))
    st = L.lib().o3dmi_pointcloud_compute_metrics(
        L.ptr(a), len(p1), L.ptr(b), len(p2), CODE[dtype],
        (C.c_int * max(len(metrics), 1))(*metrics), len(metrics),
        (C.c_float * max(r, 1))(*[float(x) for x in radii]), r, values, cap,
        C.byref(raw), None)
    return st, np.array(list(values), np.float32), dict(
        sum=list(raw.sum), max=list(raw.max),
        counts=[list(counts)[:r], list(counts)[r:2 * r]],
        second_pass=list(raw.second_pass_queries))


def untouched(values, raw):
    return ((values == np.float32(POISON)).all()
            and raw["sum"] + raw["max"] == [POISON] * 4
            and raw["second_pass"] == [-9, -9]
            and all(c == -9 for c in raw["counts"][0] + raw["counts"][1]))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        a.tobytes() == b.tobytes()


def check_pair(p1, p2, metrics=ALL, radii=RADII):
    """Both calls against the oracle; -> (values, raw) of the library."""
    want, r = orc.compute_metrics(p1, p2, metrics, radii)
    st, d12, i12 = abi_nearest(p2, p1)
    assert st == 0
    assert same_bits(d12, r["d12"])
    assert same_bits(i12, r["i12"])
    st, d21, i21 = abi_nearest(p1, p2)
    assert st == 0
    assert same_bits(d21, r["d21"])
    assert same_bits(i21, r["i21"])
    st, values, raw = abi_metrics(p1, p2, metrics, radii)
    assert st == 0
    assert same_bits(np.array(raw["sum"]), np.array(r["sum"], np.float64))
    assert same_bits(np.array(raw["max"]), np.array(r["max"], np.float64))
    assert raw["counts"] == r["counts"]
    assert same_bits(values, want)
    return values, raw


def rand_cloud(n, seed, dtype, lo=0.0, hi=1.0):
    rng = np.random.RandomState(seed)
    return (lo + (hi - lo) * rng.rand(n, 3)).astype(dtype)


# ---- upstream's vector -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_golden_cube(dtype):
    c = orc.reference_vectors()["cube"]
    p1 = np.array(c["points1"], dtype)
    p2 = p1 * dtype(c["points2_scale"])
    codes = [orc.METRIC_CODES[m] for m in c["metrics"]]
    values, raw = check_pair(p1, p2, codes, c["fscore_radius"])
    np.testing.assert_allclose(values, c["expected"], rtol=c["rtol"])
    assert raw["counts"][0] == [1, 4, 7, 8]


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_clouds(dtype):
    p = rand_cloud(1000, 1, dtype)
    values, raw = check_pair(p, p.copy())
    assert values.tolist() == [0.0, 0.0, 100.0, 100.0, 100.0, 100.0]
    assert raw["sum"] == [0.0, 0.0] and raw["max"] == [0.0, 0.0]
    st, d, i = abi_nearest(p, p)
    assert (d == 0).all() and i.tolist() == list(range(1000))


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_equal_to_a_distance_is_not_counted(dtype):
    # distances 0.5, 0.25 and 0.75, all exact in both dtypes
    target = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], dtype)
    queries = np.array([[0.5, 0, 0], [10, 0.25, 0], [0, 10, -0.75]], dtype)
    st, d, _ = abi_nearest(target, queries)
    assert st == 0 and d.tolist() == [0.5, 0.25, 0.75]
    radii = (0.5, 0.25, 0.75, np.nextafter(np.float32(0.5), np.float32(1)))
    _, raw = check_pair(queries, target, ALL, radii)
    assert raw["counts"][0] == [1, 0, 2, 2]


# ---- lane-group, wave and workgroup edges ------------------------------------------------
@functools.lru_cache(maxsize=None)
def target300(dtype):
    return rand_cloud(300, 300, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q", [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256,
                               257])
def test_query_counts_at_the_group_wave_and_workgroup_edges(q, dtype):
    check_pair(rand_cloud(q, q, dtype, -0.2, 1.2), target300(dtype))


# ---- first and second level of the sum tree ---------------------------------------------
@functools.lru_cache(maxsize=None)
def target64(dtype):
    return rand_cloud(64, 64, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q", [511, 512, 513, 262143, 262144, 262145])
def test_sum_tree_levels(q, dtype):
    check_pair(rand_cloud(q, q, dtype, -0.5, 1.5), target64(dtype))


# ---- single-level index, zero extents -----------------------------------------------------
def _degenerate(name, dtype):
    rng = np.random.RandomState(17)
    if name in ("n1", "n2", "n5"):
        return rand_cloud(int(name[1:]), 5, dtype)
    if name == "coincident":
        return np.tile(np.array([[0.25, -1.5, 3.0]], dtype), (500, 1))
    if name == "collinear":
        t = rng.rand(400, 1)
        return (t * np.array([[1.0, 2.0, -0.5]])).astype(dtype)
    if name == "coplanar":
        uv = rng.rand(600, 2)
        return np.concatenate([uv, np.full((600, 1), 0.75)], 1).astype(dtype)
    raise KeyError(name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["n1", "n2", "n5", "coincident", "collinear",
                                  "coplanar"])
def test_small_and_flat_targets(name, dtype):
    check_pair(rand_cloud(333, 9, dtype, -1.0, 2.0), _degenerate(name, dtype))


# ---- exact ties -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_ties_go_to_the_lowest_index(dtype):
    g = np.arange(6, dtype=np.float64)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    # shuffled, so that the lowest index is not the first cell visited
    lattice = lattice[np.random.RandomState(2).permutation(len(lattice))]
    h = np.arange(5, dtype=np.float64) + 0.5
    half = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    target, queries = lattice.astype(dtype), half.astype(dtype)
    d, i = orc.nearest_distance(queries, target)
    assert (d == dtype(np.sqrt(dtype(0.75)))).all()
    d2 = ((queries[:, None, :] - target[None, :, :]) ** 2).sum(-1)
    assert ((d2 == 0.75).sum(1) == 8).all()          # 8-way ties everywhere
    check_pair(queries, target)


# ---- the second pass, in both of its forms -------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_case(dtype):
    rng = np.random.RandomState(23)
    outliers = (np.array([[50.0, 50.0, 50.0]]) + rng.rand(5, 3)).astype(dtype)
    target = np.concatenate([rand_cloud(2000, 21, dtype), outliers])
    queries = np.concatenate([rand_cloud(500, 22, dtype),
                              rand_cloud(200, 24, dtype, -100.0, 100.0),
                              outliers])
    return queries, target


@pytest.mark.parametrize("dtype", DTYPES)
def test_far_queries_take_the_second_pass_in_both_forms(dtype, monkeypatch):
    queries, target = far_case(dtype)
    monkeypatch.delenv("O3DMI_KNN_SWEEP_LIMIT", raising=False)
    v_sweep, raw_sweep = check_pair(queries, target)
    assert raw_sweep["second_pass"][0] > 0
    monkeypatch.setenv("O3DMI_KNN_SWEEP_LIMIT", "0")
    v_pyr, raw_pyr = check_pair(queries, target)
    assert raw_pyr["second_pass"][0] > 0
    assert same_bits(v_sweep, v_pyr)
    assert raw_sweep == raw_pyr


# ---- a large offset ------------------------------------------------------------------------
def test_offset_cloud_float32():
    g = np.arange(12, dtype=np.float64) * 0.05
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    target = (grid + 1000.0).astype(np.float32)
    rng = np.random.RandomState(31)
    queries = (grid[rng.permutation(len(grid))[:900]] + 1000.0 +
               0.02 * rng.standard_normal((900, 3))).astype(np.float32)
    check_pair(queries, target, ALL, (0.01, 0.02, 0.05))


# ---- directions ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_directions_are_not_swapped(dtype):
    p1 = rand_cloud(700, 41, dtype)
    p2 = rand_cloud(1300, 42, dtype, 0.1, 1.3)
    radii = (0.05, 0.1)
    _, ab = check_pair(p1, p2, ALL, radii)
    _, ba = check_pair(p2, p1, ALL, radii)
    assert ab["sum"] == ba["sum"][::-1] and ab["sum"][0] != ab["sum"][1]
    assert ab["max"] == ba["max"][::-1]
    assert ab["counts"] == ba["counts"][::-1]
    assert ab["counts"][0] != ab["counts"][1]
    st, v_ab, _ = abi_metrics(p1, p2, [orc.CHAMFER], radii)
    st2, v_ba, _ = abi_metrics(p2, p1, [orc.CHAMFER], radii)
    assert st == 0 == st2 and same_bits(v_ab, v_ba)   # Chamfer is symmetric


# ---- output layout, radius groups -----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_radii", [1, 19])
def test_layout_and_radius_groups(n_radii, dtype):
    p1 = rand_cloud(900, 51, dtype)
    p2 = rand_cloud(800, 52, dtype)
    radii = tuple(0.01 + 0.007 * k for k in range(n_radii))
    v_twice, raw = check_pair(p1, p2, [orc.FSCORE, orc.CHAMFER, orc.FSCORE],
                              radii)
    assert len(v_twice) == 2 * n_radii + 1
    assert same_bits(v_twice[:n_radii], v_twice[n_radii + 1:])
    v_rev, _ = check_pair(p1, p2, ALL[::-1], radii)
    v_fwd, _ = check_pair(p1, p2, ALL, radii)
    assert same_bits(v_rev[:n_radii], v_fwd[2:])
    assert same_bits(v_rev[n_radii:], v_fwd[:2][::-1])
    if n_radii > 1:
        assert raw["counts"][0] == sorted(raw["counts"][0])
        assert raw["counts"][0][0] < raw["counts"][0][-1]


def test_the_same_call_twice_gives_the_same_bits():
    p1 = rand_cloud(5000, 61, np.float32)
    p2 = rand_cloud(4000, 62, np.float32)
    a = abi_metrics(p1, p2)
    b = abi_metrics(p1, p2)
    assert a[0] == 0 == b[0]
    assert same_bits(a[1], b[1]) and a[2] == b[2]
    da, db = abi_nearest(p2, p1), abi_nearest(p2, p1)
    assert same_bits(da[1], db[1]) and same_bits(da[2], db[2])


# ---- errors -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_leave_every_output_alone(dtype):
    good = rand_cloud(100, 71, dtype)
    for bad_value in (np.nan, np.inf):
        bad = good.copy()
        bad[37, 1] = bad_value
        for p1, p2 in ((bad, good), (good, bad)):
            st, values, raw = abi_metrics(p1, p2)
            assert st == INVALID_ARG and untouched(values, raw)
            st, d, i = abi_nearest(p2, p1)
            assert st == INVALID_ARG
            assert (d == POISON).all() and (i == -9).all()
    empty = good[:0]
    for p1, p2 in ((empty, good), (good, empty)):
        st, values, raw = abi_metrics(p1, p2)
        assert st == INVALID_ARG and untouched(values, raw)
    st, d, i = abi_nearest(empty, good)
    assert st == INVALID_ARG and (d == POISON).all() and (i == -9).all()
    st, values, raw = abi_metrics(good, good, [orc.CHAMFER, 3])
    assert st == INVALID_ARG and untouched(values, raw)
    st, values, raw = abi_metrics(good, good, ALL, ())
    assert st == INVALID_ARG and untouched(values, raw)
    st, values, raw = abi_metrics(good, good, ALL, RADII, capacity=5)
    assert st == CAPACITY and untouched(values, raw)
    # no queries: nothing to do, nothing written
    st, d, i = abi_nearest(good, empty)
    assert st == 0 and len(d) == 0


# ---- the Python mirror ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_python_mirror(dtype):
    pc = _pc()
    p1 = rand_cloud(700, 81, dtype)
    p2 = rand_cloud(900, 82, dtype)
    a1, a2 = {"positions": _dev(p1)}, {"positions": _dev(p2)}
    metrics = (pc.Metric.ChamferDistance, pc.Metric.HausdorffDistance,
               pc.Metric.FScore)
    assert metrics == tuple(ALL)
    out, raw = pc.compute_metrics(a1, a2, metrics, fscore_radius=RADII,
                                  return_raw=True)
    assert out.device.type == "cpu" and out.dtype == torch.float32
    st, values, raw_abi = abi_metrics(p1, p2)
    assert st == 0 and same_bits(out.numpy(), values)
    assert raw["sum"] == raw_abi["sum"] and raw["max"] == raw_abi["max"]
    assert raw["counts"] == raw_abi["counts"]
    assert raw["second_pass_queries"] == raw_abi["second_pass"]
    only = pc.compute_metrics(a1, a2, [pc.Metric.FScore])
    assert only.shape == (1,)                         # the default radius
    dist, idx = pc.compute_point_cloud_distance(a1, a2, return_index=True)
    st, d, i = abi_nearest(p2, p1)
    assert dist.is_cuda and dist.dtype == a1["positions"].dtype
    assert idx.dtype == torch.int32
    assert same_bits(dist.cpu().numpy(), d) and same_bits(idx.cpu().numpy(), i)
    alone = pc.compute_point_cloud_distance(a1, a2)
    assert same_bits(alone.cpu().numpy(), d)
