"""The wave-per-query neighbour searches (csrc/nns.hip: GatherCells, WaveTopK,
FloorSink) on dense, tied and cell-edge neighbourhoods, against the oracle's
exhaustive forms (tests/_nns_cases.py; the input conditions are asserted in
tests/test_nns_cases_cpu.py).

What the cases reach that the room-surface cloud of test_normals_gpu.py /
test_icp_gpu.py does not: full lists (the cut to the first max_knn, the k-th
pair pruning of WaveTopK::Push), more than kCoopCap = 512 accepted candidates
for one query (a merge in the middle of a gather and pruned pushes after it),
floor rounds after a merge and with equal distances at the floor, waves that
serve a second query, distance ties at the cut, points at exactly the radius,
points on cell faces, clouds 1000 away from the origin.

Bar: counts and indices equal to the reference, squared distances identical as
bytes, padding -1 / 0 -- the bar of the older search tests. Covariances: the
derived bound of _check_covariances. Output buffers the test owns are filled
with a sentinel before every call."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import _nns_cases as nc

pytestmark = pytest.mark.gpu

DTYPES = list(nc.DTYPES)
SENTINEL = -7


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib, registration
    return _lib, registration


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # the cases are read-only


@contextlib.contextmanager
def _index(_lib, tp, radius):
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.o3dmi_nns_create(_lib.ptr(tp), tp.shape[0],
                                  TORCH_TO_O3DMI[tp.dtype], C.c_double(radius),
                                  stream(), C.byref(h)), "nns_create")
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        L.o3dmi_nns_destroy(h)


def _buffers(q, k, dtype):
    idx = torch.full((q, k), SENTINEL, dtype=torch.int32, device="cuda")
    d2 = torch.full((q, k), SENTINEL, dtype=dtype, device="cuda")
    cnt = torch.full((q,), SENTINEL, dtype=torch.int32, device="cuda")
    return idx, d2, cnt


def _hybrid(_lib, h, tq, k):
    from open3d_amd.core import stream
    idx, d2, cnt = _buffers(tq.shape[0], k, tq.dtype)
    _lib.check(_lib.lib().o3dmi_nns_hybrid_search(
        h, _lib.ptr(tq), tq.shape[0], k, _lib.ptr(idx), _lib.ptr(d2),
        _lib.ptr(cnt), stream()), "hybrid_search")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def _wide(_lib, h, tq, k, ids=None):
    """o3dmi_internal_nns_hybrid_search_wide over all rows (ids = None) or the
    rows `ids` (numpy int32) of {q, k} outputs."""
    from open3d_amd.core import stream
    fn = _lib.lib().o3dmi_internal_nns_hybrid_search_wide
    assert fn.argtypes == _lib.INTERNAL_PROTOTYPES[
        "o3dmi_internal_nns_hybrid_search_wide"][1]
    idx, d2, cnt = _buffers(tq.shape[0], k, tq.dtype)
    tids = None if ids is None else _dev(ids)
    nq = tq.shape[0] if ids is None else int(ids.shape[0])
    _lib.check(fn(h, _lib.ptr(tq), _lib.ptr(tids), nq, k, _lib.ptr(idx),
                  _lib.ptr(d2), _lib.ptr(cnt), stream()), "hybrid_search_wide")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def _assert_rows(got, want, what, rows=None):
    """Counts, indices (padding -1) and distance bytes (padding 0) of `rows`
    (default: all)."""
    gi, gd, gc = got
    wi, wd, wc = want
    if rows is not None:
        gi, gd, gc = gi[rows], gd[rows], gc[rows]
        wi, wd, wc = wi[rows], wd[rows], wc[rows]
    assert np.array_equal(gc, wc), what
    assert np.array_equal(gi, wi), what
    assert np.ascontiguousarray(gd).tobytes() == \
        np.ascontiguousarray(wd).tobytes(), what
    pad = np.arange(wi.shape[1])[None, :] >= wc[:, None]
    assert (gi[pad] == -1).all() and (gd[pad] == 0).all(), what


# (case, offset, builder arguments, the k of the public hybrid search)
HYBRID_CASES = [
    ("dense_cube", "origin", {"radius": 0.4}, (1, 2, 63, 64)),
    ("dense_cube", "far", {"radius": 0.4}, (1, 2, 63, 64)),
    ("dense_cube", "origin", {"radius": 0.25}, (1, 2, 63, 64)),
    ("dense_cube", "far", {"radius": 0.25}, (1, 2, 63, 64)),
    ("dense_cube_small", "origin", {}, (64,)),
    ("lattice", "origin", {}, (1, 7, 64)),
    ("lattice", "far", {}, (1, 7, 64)),
    ("duplicates", "origin", {}, (64,)),
    ("duplicates", "far", {}, (64,)),
    ("cell_faces", "origin", {}, (64,)),
    ("inward_tiers", "origin", {}, (1, 40, 41, 64)),
    ("inward_tiers", "far", {}, (64,)),
]


def _case_id(c):
    return "-".join([c[0], c[1]] + ["%s%s" % kv for kv in sorted(c[2].items())])


@pytest.mark.parametrize("case", HYBRID_CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hybrid_search_full_lists(dtype, case):
    """o3dmi_nns_hybrid_search, k <= 64, where the lists fill: r = 0.25 fills
    every list without a merge, r = 0.4 merges in the middle of the gather for
    most queries and prunes the pushes after it; the lattice cuts k = 64 inside
    a group of equal distances and leaves out 6 points at exactly the radius;
    the duplicates make every distance of a row equal; the inward tiers merge
    three times during one gather, the last time into a list whose 40 nearest
    entries must survive."""
    _lib, _ = _gpu()
    name, offset, extra, ks = case
    pts, qrs, radius = nc.case(name, dtype, offset, **extra)
    ref = nc.reference(name, dtype, offset, **extra)
    tp, tq = _dev(pts), _dev(qrs)
    with _index(_lib, tp, radius) as h:
        for k in ks:
            want = nc.hybrid_rows(ref, k)
            got = _hybrid(_lib, h, tq, k)
            _assert_rows(got, want, (name, offset, k))
            if name == "duplicates":
                ip, iq = nc.duplicates_groups()
                both = np.sort(np.concatenate([ip, iq]))
                assert np.array_equal(got[0][0], ip[:64])     # query P
                assert np.array_equal(got[0][1], iq[:64])     # query Q
                assert np.array_equal(got[0][2], both[:64])   # midpoint
                assert np.array_equal(got[0][3], both[:64])   # bisector
            elif name.startswith("dense_cube"):
                assert (want[2] == k).all()                   # full lists


WIDE_CASES = [("dense_cube", "origin", {"radius": 0.4}),
              ("lattice", "origin", {}),
              ("duplicates", "origin", {}),
              ("inward_tiers", "origin", {})]


@pytest.mark.parametrize("case", WIDE_CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hybrid_search_wide_floor_rounds(dtype, case):
    """o3dmi_internal_nns_hybrid_search_wide, max_knn in {65, 100, 128}: a
    second round of 1, 36 or 64 pairs above the floor (the 64th pair of the
    first round), after a merge on the dense cube, with the floor inside a
    group of equal distances on the lattice and the duplicates. Once over all
    rows, once over every third row in descending order: the rows not named
    keep the sentinel."""
    _lib, _ = _gpu()
    name, offset, extra = case
    pts, qrs, radius = nc.case(name, dtype, offset, **extra)
    ref = nc.reference(name, dtype, offset, **extra)
    tp, tq = _dev(pts), _dev(qrs)
    q = qrs.shape[0]
    ids = np.ascontiguousarray(np.arange(q, dtype=np.int32)[::3][::-1])
    rest = np.setdiff1d(np.arange(q), ids)
    with _index(_lib, tp, radius) as h:
        for k in (65, 100, 128):
            want = nc.hybrid_rows(ref, k)
            _assert_rows(_wide(_lib, h, tq, k), want, (name, k, "all rows"))
            got = _wide(_lib, h, tq, k, ids)
            _assert_rows(got, want, (name, k, "ids"), rows=ids)
            if rest.size:
                assert (got[0][rest] == SENTINEL).all(), (name, k)
                assert (got[1][rest] == SENTINEL).all(), (name, k)
                assert (got[2][rest] == SENTINEL).all(), (name, k)


RADIUS_CASES = [("dense_cube", "origin", {"radius": 0.4}),
                ("dense_cube", "far", {"radius": 0.4}),
                ("lattice", "origin", {}),
                ("duplicates", "origin", {}),
                ("cell_faces", "origin", {}),
                ("inward_tiers", "origin", {})]


@pytest.mark.parametrize("case", RADIUS_CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_radius_search_long_lists(dtype, case):
    """registration.fixed_radius_search (radius count, prefix sum, radius
    write): lists of up to 1356 on the dense cube -- more than 16 floor rounds,
    a merge in most of them --, lists of 1000 with two distinct distances on
    the duplicates (every floor sits inside a run of equal distances)."""
    _lib, reg = _gpu()
    name, offset, extra = case
    pts, qrs, radius = nc.case(name, dtype, offset, **extra)
    ref = nc.reference(name, dtype, offset, **extra)
    idx, d2, splits = reg.fixed_radius_search(_dev(pts), _dev(qrs), radius)
    splits = splits.cpu().numpy()
    assert splits[0] == 0 and np.array_equal(np.diff(splits), ref[2])
    flat_i, flat_d = nc.flat_lists(ref)
    assert np.array_equal(idx.cpu().numpy(), flat_i)
    assert d2.cpu().numpy().tobytes() == flat_d.tobytes()
    if name == "dense_cube":
        assert ref[2].max() > 1090
    if name == "duplicates":
        assert ref[2].tolist() == [1000] * 4


def _radius_covariances(_lib, h, tq):
    from open3d_amd.core import stream
    cov = torch.full((tq.shape[0], 3, 3), SENTINEL, dtype=tq.dtype,
                     device="cuda")
    _lib.check(_lib.lib().o3dmi_nns_radius_covariances(
        h, _lib.ptr(tq), tq.shape[0], _lib.ptr(cov), stream()),
        "radius_covariances")
    torch.cuda.synchronize()
    return cov.cpu().numpy()


def _check_covariances(pts, qrs, radius, got, what):
    """o3dmi_nns_radius_covariances against the covariance of the exhaustive
    neighbour set in numpy.longdouble. Fewer than 3 neighbours: the identity,
    exactly. Else, per entry (a, b), with n neighbours, u = 2^-53,
    t_i = (x_i,a - c_a)(x_i,b - c_b) about the exact centroid c and
    S = sum |t_i|:

        |got - exact| <= (n + 8) u S / (n - 1)      (+ ulp32(exact) / 2)

    Derivation. The kernel forms the centroid c' in float64, then per
    neighbour d_a = x_a - c'_a (one rounding), the product d_a d_b (one
    rounding, or none where it is fused into the sum), adds the products per
    lane and across the wave in an order that is not fixed, and divides by
    n - 1 (one rounding). A sum of n terms has relative error <= (n - 1) u of
    sum |terms| in any order (Higham, Accuracy and Stability, eq. 4.4, first
    order); each term carries <= 3 u of its own (two differences, one
    product); the division one more: (n + 3) u S / (n - 1) to first order.
    The 5 u on top cover the second-order terms and the centroid: replacing c
    by c' = c + e changes the sum by n e_a e_b exactly (the first-order terms
    vanish because sum (x_i - c) = 0), and |e| <= n u max|x|, so that change
    is <= n^3 u^2 max|x|^2 -- relative to the bound n u S ~ n^2 u var that is
    n u max|x|^2 / var, <= 1.5e-13 * 4e7 = 6e-6 of the bound at the 1000
    offset (var ~ 0.03): it disappears in the 5 u. float32 outputs
    are that float64 value rounded once more: half an ulp of the entry.
    Returns the largest |error| / bound."""
    dtype = pts.dtype
    worst = 0.0
    eye = np.eye(3, dtype=dtype)
    exact_of = {}
    n_few = 0
    for b in range(0, qrs.shape[0], 1024):
        idx, _, cnt = nc.exhaustive_radius(pts, qrs[b:b + 1024], radius)
        for r in range(cnt.shape[0]):
            c = int(cnt[r])
            g = got[b + r]
            if c < 3:
                n_few += 1
                assert g.tobytes() == eye.tobytes(), (what, b + r, c)
                continue
            key = np.sort(idx[r, :c]).tobytes()
            if key not in exact_of:
                exact, S = nc.covariance_reference(pts, idx[r], c)
                exact_of[key] = (exact, nc.covariance_bound(exact, S, c, dtype))
            exact, bound = exact_of[key]
            err = np.abs(g.astype(np.longdouble) - exact)
            assert (bound > 0).all(), (what, b + r)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert (err <= bound).all(), (what, b + r, c, ratio)
    print("covariances %s %s: largest error / bound = %.4f (%d sets, %d rows "
          "with < 3 neighbours)" % (what, np.dtype(dtype).name, worst,
                                    len(exact_of), n_few))
    return worst, n_few


@pytest.mark.parametrize("offset", list(nc.OFFSETS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_covariances_dense(dtype, offset):
    """Neighbourhoods of 314 .. 1356 points: 5 .. 22 batches of 64 per sweep
    and lane, summed in float64. Bound: _check_covariances."""
    _lib, _ = _gpu()
    pts, qrs, radius = nc.case("dense_cube", dtype, offset, radius=0.4)
    tp, tq = _dev(pts), _dev(qrs)
    with _index(_lib, tp, radius) as h:
        got = _radius_covariances(_lib, h, tq)
    _check_covariances(pts, qrs, radius, got, "dense_cube " + offset)


@pytest.mark.parametrize("sparse_first", [False, True],
                         ids=["dense_then_sparse", "sparse_then_dense"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wave_reuse_across_entry_points(dtype, sparse_first):
    """16384 + 40 queries on launches of at most 16384 waves: 40 waves serve a
    second query, of the other kind than their first (1000 neighbours, then 0
    to 3, or the other way round), through the hybrid search (k = 64), the wide
    one (k = 128), the radius count and the radius covariances. The sparse rows
    are checked first: they must be the exact short lists, padded."""
    _lib, _ = _gpu()
    from open3d_amd.core import stream
    pts, qrs, radius = nc.case("wave_reuse", dtype, sparse_first=sparse_first)
    ref = nc.reference("wave_reuse", dtype, keep=128, sparse_first=sparse_first)
    sparse = nc.wave_reuse_sparse_rows(sparse_first)
    q = qrs.shape[0]
    assert q > nc.LAUNCH_WAVES
    tp, tq = _dev(pts), _dev(qrs)
    with _index(_lib, tp, radius) as h:
        got64 = _hybrid(_lib, h, tq, 64)
        got128 = _wide(_lib, h, tq, 128)
        cnt = torch.full((q,), SENTINEL, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().o3dmi_nns_radius_count(
            h, _lib.ptr(tq), q, _lib.ptr(cnt), stream()), "radius_count")
        cov = _radius_covariances(_lib, h, tq)
    want64, want128 = nc.hybrid_rows(ref, 64), nc.hybrid_rows(ref, 128)
    _assert_rows(got64, want64, "hybrid, sparse rows", rows=sparse)
    _assert_rows(got128, want128, "wide, sparse rows", rows=sparse)
    _assert_rows(got64, want64, "hybrid")
    _assert_rows(got128, want128, "wide")
    assert np.array_equal(cnt.cpu().numpy()[sparse], ref[2][sparse])
    assert np.array_equal(cnt.cpu().numpy(), ref[2])
    _, n_few = _check_covariances(pts, qrs, radius, cov, "wave_reuse")
    assert n_few >= 25


KNN_CASES = [("lattice", "origin", {"knn_queries": True}, (1, 63, 64)),
             ("dense_cube", "origin", {}, (64,)),
             ("dense_cube", "far", {}, (64,)),
             ("duplicates", "origin", {}, (64,)),
             ("two_scales", "origin", {}, (1, 64))]


@pytest.mark.parametrize("case", KNN_CASES, ids=_case_id)
@pytest.mark.parametrize("second_pass", ["sweep", "pyramid"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_search_dense_and_tied(dtype, second_pass, case, monkeypatch):
    """registration.knn_search in both second-pass forms: the lattice with
    queries on faces, edges and corners of its cells (distance 0 to the own
    cell's nearest face) and ten extents outside; the dense cube at both
    offsets; 1000 coincident points; two scales seven orders apart with
    queries far outside everything."""
    _lib, reg = _gpu()
    monkeypatch.setenv("O3DMI_KNN_SWEEP_LIMIT",
                       "1e30" if second_pass == "sweep" else "0")
    name, offset, extra, ks = case
    pts, qrs, _ = nc.case(name, dtype, offset, **extra)
    tp, tq = _dev(pts), _dev(qrs)
    for k in ks:
        widx, wd2 = nc.knn_reference(name, dtype, k, offset, **extra)
        idx, d2 = reg.knn_search(tp, tq, k)
        assert idx.shape == (qrs.shape[0], k), (name, k)
        assert np.array_equal(idx.cpu().numpy(), widx), (name, k)
        assert d2.cpu().numpy().tobytes() == wd2.tobytes(), (name, k)


@pytest.mark.parametrize("n", [65, 40])
@pytest.mark.parametrize("second_pass", ["sweep", "pyramid"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_search_k_next_to_the_cloud_size(dtype, second_pass, n,
                                             monkeypatch):
    """k = 64 on 65 points (all but one point of the cloud in every row) and
    on 40 points (40 columns: the whole cloud, sorted)."""
    import _oracle as orc
    _lib, reg = _gpu()
    monkeypatch.setenv("O3DMI_KNN_SWEEP_LIMIT",
                       "1e30" if second_pass == "sweep" else "0")
    pts, qrs, _ = nc.small_cloud(dtype, n)
    widx, wd2 = orc.knn_search(pts, qrs, 64)
    idx, d2 = reg.knn_search(_dev(pts), _dev(qrs), 64)
    assert idx.shape == (50, min(n, 64)) == widx.shape
    assert np.array_equal(idx.cpu().numpy(), widx)
    assert d2.cpu().numpy().tobytes() == wd2.tobytes()
