"""CPU checks of the metrics oracle (tests/_pointcloud_metrics_oracle.py)
against upstream's own vector, of the library's pure host function
o3dmi_metrics_from_sums against the oracle's final arithmetic, bit for bit, and
of every argument error the new calls answer before their first launch.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import _pointcloud_metrics_oracle as orc

INVALID_ARG, CAPACITY = 1, 3
F32, F64, I32 = 0, 1, 4
FAKE = C.c_void_p(0x1000)  # never dereferenced: the checks come first
POISON = -777.0


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from open3d_amd import _lib
    _lib.lib()
    return _lib


def cube(dtype):
    c = orc.reference_vectors()["cube"]
    p1 = np.array(c["points1"], dtype)
    p2 = p1 * dtype(c["points2_scale"])
    return c, p1, p2


# ---- the oracle against upstream's vector -----------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_matches_the_golden_cube(dtype):
    c, p1, p2 = cube(dtype)
    codes = [orc.METRIC_CODES[m] for m in c["metrics"]]
    got, r = orc.compute_metrics(p1, p2, codes, c["fscore_radius"])
    assert got.dtype == np.float32 and got.shape == (6,)
    np.testing.assert_allclose(got, c["expected"], rtol=c["rtol"])
    assert r["i12"].tolist() == list(range(8)) == r["i21"].tolist()
    assert r["counts"][0] == [1, 4, 7, 8]


def test_golden_cube_float32_values_are_the_ones_the_issue_states():
    c, p1, p2 = cube(np.float32)
    got, _ = orc.compute_metrics(p1, p2, [0, 1, 2], c["fscore_radius"])
    assert ["%.8g" % v for v in got] == ["0.22436735", "0.17320512", "12.5",
                                         "50", "87.5", "100"]


def test_tree_sum_is_runs_of_512_level_by_level():
    v = np.random.RandomState(3).rand(512 * 513 + 7).astype(np.float32)
    runs = []
    for s in range(0, len(v), orc.RUN):
        acc = np.float64(v[s])
        for x in v[s + 1:s + orc.RUN]:
            acc = acc + np.float64(x)
        runs.append(acc)
    level2 = []
    for s in range(0, len(runs), orc.RUN):
        acc = runs[s]
        for x in runs[s + 1:s + orc.RUN]:
            acc = acc + x
        level2.append(acc)
    assert len(level2) == 2
    assert orc.tree_sum(v) == level2[0] + level2[1]
    assert orc.tree_sum(v[:1]) == np.float64(v[0])


def test_nearest_ties_go_to_the_lowest_index():
    t = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 0], [0, 0, 0]],
                 np.float32)
    d, i = orc.nearest_distance(np.array([[0, 0, 0], [0, 0, 2]], np.float32),
                                t)
    assert i.tolist() == [3, 3] and d.tolist() == [0.0, 2.0]


# ---- o3dmi_metrics_from_sums -----------------------------------------------------
def from_sums(L, n1, n2, sums, maxs, counts, metrics, capacity=None,
              n_radii=None):
    r = len(counts[0]) if n_radii is None else n_radii
    flat = list(counts[0]) + list(counts[1])
    n_values = sum(r if m == 2 else 1 for m in metrics)
    cap = n_values if capacity is None else capacity
    out = (C.c_float * max(cap, 1))(*([POISON] * max(cap, 1)))
    st = L.lib().o3dmi_metrics_from_sums(
        n1, n2, (C.c_double * 2)(*sums), (C.c_double * 2)(*maxs),
        (C.c_int64 * max(len(flat), 1))(*flat), r,
        (C.c_int * max(len(metrics), 1))(*metrics), len(metrics), out, cap)
    return st, np.array(list(out), np.float32)


HAND_MADE = [
    # n1, n2, sums, maxs, counts12, counts21
    (8, 8, [0.9, 0.8949389], [0.17320508, 0.1732051], [1, 4, 7, 8],
     [1, 4, 7, 8]),
    (700, 1300, [12.345678901234, 98.7654321], [0.5, 0.25], [0, 3, 700],
     [0, 0, 1300]),                      # precision + recall = 0; a count of 0
    (3, 7, [1e-30, 3.3e20], [1e-40, 7.7e19], [0], [5]),
    (3, 7, [0.1, 0.2], [0.3, 0.1], [2], [0]),
    ((1 << 24) + 3, 5, [123456.789, 1.5], [3.0, 4.0], [(1 << 24) + 1], [2]),
    (1, 1, [0.0, 0.0], [0.0, 0.0], [1], [1]),
]


@pytest.mark.parametrize("case", range(len(HAND_MADE)))
@pytest.mark.parametrize("metrics", [[0, 1, 2], [2, 1, 0], [2, 2], [1], []])
def test_metrics_from_sums_is_the_oracle_bit_for_bit(L, case, metrics):
    n1, n2, sums, maxs, c12, c21 = HAND_MADE[case]
    st, got = from_sums(L, n1, n2, sums, maxs, [c12, c21], metrics)
    assert st == 0
    want = orc.values_from_sums(n1, n2, sums, maxs, [c12, c21], metrics)
    assert got[:len(want)].tobytes() == want.tobytes()


def test_fscore_is_zero_when_precision_and_recall_are():
    got = orc.values_from_sums(700, 1300, [1.0, 1.0], [1.0, 1.0], [[0], [0]],
                               [2])
    assert got.tolist() == [0.0]


def test_metrics_from_sums_errors_leave_the_values_alone(L):
    ok = (8, 8, [1.0, 1.0], [1.0, 1.0], [[1], [1]])
    for bad, metrics, kw in [
            ((0,) + ok[1:], [0], {}),                 # empty cloud
            ((8, -1) + ok[2:], [0], {}),
            (ok, [3], {}),                            # unknown code
            (ok, [0, -1], {}),
            (ok[:4] + ([[], []],), [2], {}),          # FScore without radii
            (ok, [0], {"n_radii": -1}),
    ]:
        st, out = from_sums(L, *bad, metrics, **kw)
        assert st == INVALID_ARG, (bad, metrics)
        assert (out == np.float32(POISON)).all()
    st, out = from_sums(L, *ok, [0, 2, 1], capacity=2)
    assert st == CAPACITY and (out == np.float32(POISON)).all()
    lib = L.lib()
    two = (C.c_double * 2)(1.0, 1.0)
    one = (C.c_int * 1)(0)
    val = (C.c_float * 1)(POISON)
    assert lib.o3dmi_metrics_from_sums(8, 8, None, two, None, 0, one, 1, val,
                                       1) == INVALID_ARG
    assert lib.o3dmi_metrics_from_sums(8, 8, two, two, None, 0, None, 1, val,
                                       1) == INVALID_ARG
    assert lib.o3dmi_metrics_from_sums(8, 8, two, two, None, 0, one, 1, None,
                                       1) == INVALID_ARG
    assert val[0] == POISON


# ---- argument errors of the device calls, all before the first launch ---------------
def test_nearest_distance_argument_errors(L):
    f = L.lib().o3dmi_pointcloud_nearest_distance
    assert f(FAKE, 0, FAKE, 5, F32, FAKE, None, None) == INVALID_ARG  # empty
    assert f(FAKE, -1, FAKE, 5, F32, FAKE, None, None) == INVALID_ARG
    assert f(FAKE, 5, FAKE, -1, F32, FAKE, None, None) == INVALID_ARG
    assert f(None, 5, FAKE, 5, F32, FAKE, None, None) == INVALID_ARG
    assert f(FAKE, 5, None, 5, F32, FAKE, None, None) == INVALID_ARG
    assert f(FAKE, 5, FAKE, 5, F32, None, None, None) == INVALID_ARG
    assert f(FAKE, 5, FAKE, 5, I32, FAKE, None, None) == INVALID_ARG
    assert f(FAKE, 1 << 31, FAKE, 5, F32, FAKE, None, None) == INVALID_ARG
    assert f(FAKE, 5, FAKE, (1 << 31) - 1, F64, FAKE, None, None) == INVALID_ARG


def test_compute_metrics_argument_errors(L):
    f = L.lib().o3dmi_pointcloud_compute_metrics
    counts = (C.c_int64 * 4)(-9, -9, -9, -9)
    raw = L.MetricsRawC()
    raw.sum[0] = raw.sum[1] = raw.max[0] = raw.max[1] = POISON
    raw.second_pass_queries[0] = raw.second_pass_queries[1] = -9
    raw.counts = C.cast(counts, C.POINTER(C.c_int64))
    values = (C.c_float * 8)(*([POISON] * 8))
    radii = (C.c_float * 2)(0.1, 0.2)

    def call(p1=FAKE, n1=5, p2=FAKE, n2=6, dtype=F32, metrics=(0, 1, 2),
             n_metrics=None, fr=radii, n_radii=2, out=values, cap=8):
        codes = (C.c_int * max(len(metrics), 1))(*metrics)
        return f(p1, n1, p2, n2, dtype, codes if metrics else None,
                 len(metrics) if n_metrics is None else n_metrics, fr, n_radii,
                 out, cap, C.byref(raw), None)

    assert call(n1=0) == INVALID_ARG                  # an empty cloud
    assert call(n2=0) == INVALID_ARG
    assert call(n1=-3) == INVALID_ARG
    assert call(p1=None) == INVALID_ARG
    assert call(p2=None) == INVALID_ARG
    assert call(dtype=I32) == INVALID_ARG
    assert call(metrics=(0, 3)) == INVALID_ARG        # unknown code
    assert call(metrics=(-1,)) == INVALID_ARG
    assert call(n_radii=0) == INVALID_ARG             # FScore with no radii
    assert call(n_radii=-1) == INVALID_ARG
    assert call(fr=None) == INVALID_ARG
    assert call(out=None) == INVALID_ARG
    assert call(metrics=(), n_metrics=2) == INVALID_ARG
    assert call(n_metrics=-1) == INVALID_ARG
    assert call(n1=1 << 31) == INVALID_ARG
    assert call(cap=3) == CAPACITY                    # 1 + 1 + 2 values
    assert call(metrics=(2, 2), cap=3) == CAPACITY    # FScore expands twice
    assert list(values) == [POISON] * 8
    assert list(counts) == [-9] * 4
    assert list(raw.sum) + list(raw.max) == [POISON] * 4
    assert list(raw.second_pass_queries) == [-9, -9]


def test_the_table_binds_the_new_symbols(L):
    for name in ("o3dmi_pointcloud_nearest_distance",
                 "o3dmi_pointcloud_compute_metrics",
                 "o3dmi_metrics_from_sums"):
        assert name in L.PROTOTYPES
        assert hasattr(L.lib(), name)
