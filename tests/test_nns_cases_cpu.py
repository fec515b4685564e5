"""The input conditions tests/test_nns_dense_gpu.py relies on, asserted without
a GPU, so that a changed seed or constant cannot silently empty a case; and
the exhaustive reference of tests/_nns_cases.py against a plain numpy
restatement, bit for bit."""
import numpy as np
import pytest

import _nns_cases as nc

DTYPES = list(nc.DTYPES)
OFFSETS = list(nc.OFFSETS)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_cube_fills_lists_and_forces_merges(dtype, offset):
    pts, qrs, _ = nc.case("dense_cube", dtype, offset, radius=0.4)
    assert pts.shape == (5000, 3) and pts.shape[0] > nc.SMALL_INDEX_POINTS
    assert qrs.shape == (300, 3) and pts.dtype == dtype == qrs.dtype
    # negative and positive cell coordinates about the offset
    rel = pts.astype(np.float64) - np.asarray(nc.OFFSETS[offset])
    assert (rel.min(0) < -0.1).all() and (rel.max(0) > 0.1).all()
    cnt = nc.reference("dense_cube", dtype, offset, radius=0.4)[2]
    # a merge in the middle of a gather: more than kCoopCap accepted
    assert (cnt >= nc.K_COOP_CAP + 1).mean() >= 0.5
    # more than 16 floor rounds of 64, several after merges
    assert (cnt >= 1090).mean() >= 0.10
    cnt = nc.reference("dense_cube", dtype, offset, radius=0.25)[2]
    # full lists without a merge
    assert cnt.min() >= 64 and cnt.max() <= nc.K_COOP_CAP


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_cube_small_uses_the_small_index(dtype):
    pts, qrs, radius = nc.case("dense_cube_small", dtype)
    assert pts.shape == (3000, 3) and pts.shape[0] <= nc.SMALL_INDEX_POINTS
    assert radius == 0.4
    cnt = nc.reference("dense_cube_small", dtype)[2]
    assert cnt.min() >= 64 and cnt.max() > nc.K_COOP_CAP


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_ties_and_points_at_the_radius(dtype, offset):
    pts, qrs, radius = nc.case("lattice", dtype, offset)
    assert pts.shape == (4913, 3) and radius == 0.25
    # every coordinate is exact in the point dtype
    c = np.arange(-8, 9) * nc.LATTICE_STEP
    g = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(pts.astype(np.float64),
                          g + np.asarray(nc.OFFSETS[offset]))
    idx, d2, cnt = nc.reference("lattice", dtype, offset)
    near = d2[0, :cnt[0]]
    assert cnt[0] > 200 and np.unique(near).size < 20
    # k = 64 cuts inside a tie group: the index decides
    assert near[63] == near[64] and idx[0, 63] < idx[0, 64]
    assert near[62] == near[63]
    # exactly 6 points at d2 == r^2, all excluded (strict <)
    all_d2, _ = nc.numpy_sorted_pairs(pts, qrs[0])
    r2 = dtype(radius) * dtype(radius)
    assert int((all_d2 == r2).sum()) == 6
    assert int((all_d2 < r2).sum()) == cnt[0]
    # the same d2 whatever the offset: the lattice is exact there too
    assert np.array_equal(d2, nc.reference("lattice", dtype, "origin")[1])


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_counts_and_exact_equidistance(dtype, offset):
    pts, qrs, radius = nc.case("duplicates", dtype, offset)
    ip, iq = nc.duplicates_groups()
    assert ip.size == 700 and iq.size == 300 and radius == 0.2
    assert int((pts == qrs[0]).all(1).sum()) == 700
    assert int((pts == qrs[1]).all(1).sum()) == 300
    assert np.array_equal(np.where((pts == qrs[0]).all(1))[0], ip)
    assert np.array_equal(np.where((pts == qrs[1]).all(1))[0], iq)
    # interleaved, not grouped: both groups start within the first few indices
    assert ip[0] == 0 and iq[0] == 4 and ip[-1] == 1998 and iq[-1] == 1996
    assert np.linalg.norm(nc.DUP_P - nc.DUP_Q) < 0.05
    idx, d2, cnt = nc.reference("duplicates", dtype, offset)
    # the background is out of range of every query
    assert cnt.tolist() == [1000] * 4 and not (idx[:, :1000] % 2).any()
    # P: 700 at d2 = 0, then Q's 300; Q: the other way round
    assert np.array_equal(idx[0, :700], ip) and np.array_equal(idx[0, 700:], iq)
    assert np.array_equal(idx[1, :300], iq) and np.array_equal(idx[1, 300:], ip)
    assert np.unique(d2[0]).size == 2 and np.unique(d2[1]).size == 2
    # midpoint and bisector query: one distance, index order over both groups
    both = np.sort(np.concatenate([ip, iq]))
    for row in (2, 3):
        assert np.unique(d2[row]).size == 1
        assert np.array_equal(idx[row], both)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cell_faces_sit_on_the_faces(dtype):
    pts, qrs, radius = nc.case("cell_faces", dtype)
    assert radius == 0.125
    cell = radius * 1.001
    n_face = qrs.shape[0]
    assert n_face == 3 * 21 * 3 + 42 and pts.shape[0] == n_face + 2000
    assert np.array_equal(pts[:n_face], qrs)
    # per face: the value itself and its two neighbours in the point dtype
    x = qrs[:21 * 3:3, 0]
    for j in range(-3, 4):
        v = dtype(j * cell)
        trio = x[3 * (j + 3):3 * (j + 3) + 3]
        assert trio[1] == v
        assert trio[0] == np.nextafter(v, dtype(-np.inf)) and trio[0] < v
        assert trio[2] == np.nextafter(v, dtype(np.inf)) and trio[2] > v
    cnt = nc.reference("cell_faces", dtype)[2]
    assert cnt.min() >= 3        # each face point sees its two neighbours


@pytest.mark.parametrize("dtype", DTYPES)
def test_inward_tiers_force_merges_into_a_full_list(dtype):
    """The conditions under which WaveTopK merges three times during one
    gather, the third time with the 40 nearest points in its list: the four
    groups lie in four cells of rising gather order and their distance ranges
    are disjoint, A > C > D > B, all within the radius."""
    pts, qrs, radius = nc.case("inward_tiers", dtype)
    cell = radius * 1.001
    bounds = np.cumsum((0,) + nc.TIER_SIZES)
    assert pts.shape[0] == bounds[-1] <= nc.SMALL_INDEX_POINTS
    order, lo, hi = [], [], []
    for q in qrs:
        qc = np.floor(q.astype(np.float64) / cell)
        assert qc.tolist() == [0, 0, 0]
        for t in range(4):
            p = pts[bounds[t]:bounds[t + 1]].astype(np.float64)
            pc = np.floor(p / cell)
            assert (pc == np.asarray(nc.TIER_CELLS[t])).all()
            d = np.linalg.norm(p - q.astype(np.float64), axis=1)
            lo.append(d.min())
            hi.append(d.max())
        order.append([(c[0] + 1) + 3 * (c[1] + 1) + 9 * (c[2] + 1)
                      for c in nc.TIER_CELLS])
    assert all(o == sorted(o) and len(set(o)) == 4 for o in order)
    lo, hi = np.array(lo).reshape(-1, 4), np.array(hi).reshape(-1, 4)
    a, b, c, d = range(4)
    assert (hi[:, b] < lo[:, d]).all() and (hi[:, d] < lo[:, c]).all()
    assert (hi[:, c] < lo[:, a]).all() and (hi[:, a] < radius * 0.99).all()
    # each of A, C and D alone overflows the buffer of kCoopCap + 64
    assert min(nc.TIER_SIZES[a], nc.TIER_SIZES[c],
               nc.TIER_SIZES[d]) > nc.K_COOP_CAP + 64
    assert nc.TIER_SIZES[b] < 64
    idx, _, cnt = nc.reference("inward_tiers", dtype)
    assert (cnt == bounds[-1]).all()
    # the 64 nearest: all of B, then D
    first = np.sort(idx[:, :64], axis=1)
    assert np.array_equal(first[:, :40], np.tile(np.arange(600, 640), (4, 1)))
    assert (first[:, 40:] >= bounds[3]).all()


@pytest.mark.parametrize("sparse_first", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wave_reuse_has_more_queries_than_waves(dtype, sparse_first):
    pts, qrs, radius = nc.case("wave_reuse", dtype, sparse_first=sparse_first)
    assert pts.shape == (2000, 3) and radius == 0.12
    assert qrs.shape[0] == nc.LAUNCH_WAVES + 40
    assert (np.linalg.norm(pts[:1000].astype(np.float64), axis=1)
            <= 0.05 + 1e-6).all()
    idx, d2, cnt = nc.reference("wave_reuse", dtype, keep=128,
                                sparse_first=sparse_first)
    rows = nc.wave_reuse_sparse_rows(sparse_first)
    dense = np.delete(np.arange(qrs.shape[0]), rows)
    assert dense.size == nc.LAUNCH_WAVES
    assert (np.linalg.norm(qrs[dense].astype(np.float64), axis=1)
            <= 0.02 + 1e-6).all()
    assert cnt[dense].min() >= 1000
    sparse = cnt[rows]
    assert sparse.max() <= 8 and (sparse == 0).sum() >= 10
    assert (sparse >= 3).sum() >= 5 and ((sparse > 0) & (sparse < 3)).any()
    # a wave's second query is of the other kind: wave w serves w and
    # w + 16384, and the last 40 queries are the first 40's partners
    first = np.arange(40)
    assert (np.isin(first, rows) != np.isin(first + nc.LAUNCH_WAVES, rows)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_scales_and_small_clouds(dtype):
    pts, qrs, radius = nc.case("two_scales", dtype)
    assert radius is None and pts.shape == (6001, 3) and qrs.shape == (203, 3)
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    assert (r[:3000] <= 1e-3 * (1 + 1e-6)).all() and r[-1] > 1.7e4
    assert np.abs(pts[3000:6000]).max() <= 50
    assert qrs[-1].tolist() == [55.0, 0.0, 0.0]
    for n in (65, 40):
        p, q, _ = nc.small_cloud(dtype, n)
        assert p.shape == (n, 3) and q.shape == (50, 3) and p.dtype == dtype


@pytest.mark.parametrize("name", ["lattice", "dense_cube_small"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_reference_equals_numpy_restatement(dtype, name):
    """d2 = ((dx dx) + dy dy) + dz dz in the point dtype, dx = query - point,
    stable sort by (d2, index), strict d2 < T(radius)^2: the same bytes as the
    oracle's exhaustive form. (The oracle's grid form agrees too, but is not
    the reference.)"""
    import _oracle as orc
    pts, qrs, radius = nc.case(name, dtype)
    if name == "dense_cube_small":
        qrs = qrs[::6]
    idx, d2, cnt = nc.exhaustive_radius(pts, qrs, radius)
    width = idx.shape[1]
    assert width == cnt.max()
    nidx, nd2, ncnt = nc.numpy_radius_rows(pts, qrs, radius, width)
    assert np.array_equal(cnt, ncnt)
    assert np.array_equal(idx, nidx)
    assert d2.tobytes() == nd2.tobytes()
    # hybrid rows cut from it == the oracle called with that max_knn
    for k in (1, 64, 100):
        want = orc.hybrid_search(pts, qrs, radius, k, brute=True)
        got = nc.hybrid_rows((idx, d2, cnt), k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2],
                                                                  want[2])
        assert got[1].tobytes() == want[1].tobytes()
        grid = orc.hybrid_search(pts, qrs, radius, k)
        assert np.array_equal(grid[0], want[0])
    # KNN: the first k of the sorted pairs of the whole cloud
    kidx, kd2 = orc.knn_search(pts, qrs, 64)
    for i in range(qrs.shape[0]):
        sd, si = nc.numpy_sorted_pairs(pts, qrs[i])
        assert np.array_equal(kidx[i], si[:64])
        assert kd2[i].tobytes() == sd[:64].tobytes()


def test_covariance_reference_of_a_known_set():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 2, 0]], np.float64)
    idx = np.arange(4, dtype=np.int32)
    exact, S = nc.covariance_reference(pts, idx, 4)
    assert np.allclose(exact.astype(np.float64),
                       np.cov(pts.T), rtol=0, atol=1e-15)
    assert float(S[0, 0]) == 1.0 and float(S[1, 1]) == 4.0
    assert float(S[0, 1]) == 2.0 and float(exact[0, 1]) == 0.0
    b = nc.covariance_bound(exact, S, 4, np.float64)
    assert float(b[0, 0]) == 12 * 2.0 ** -53 * 1.0 / 3
