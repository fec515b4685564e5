"""FPFH features and feature correspondences on the MI355X against the numpy
restatement (tests/_fpfh_oracle.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _fpfh_oracle as fo
import _oracle as orc
from _seam_cases import surface as _surface

pytestmark = pytest.mark.gpu


def _reg():
    from open3d_amd import registration
    return registration


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle_full(pts, nrm, mode, max_nn, radius, edge_tol=None):
    if mode == "hybrid":
        idx, d2, cnt = orc.hybrid_search(pts, pts, radius, max_nn)
        return fo.fpfh_from_lists(pts, nrm, idx, d2, counts=cnt,
                                  edge_tol=edge_tol)
    if mode == "knn":
        idx, d2 = orc.knn_search(pts, pts, max_nn)
        cnt = np.full(pts.shape[0], idx.shape[1], np.int32)
        return fo.fpfh_from_lists(pts, nrm, idx, d2, counts=cnt,
                                  edge_tol=edge_tol)
    idx, d2, splits = fo.radius_lists(pts, radius)
    return fo.fpfh_from_lists(pts, nrm, idx, d2, splits=splits,
                              edge_tol=edge_tol)


def _check_f32(got, want, flagged):
    """Float32 rows match the restatement except rows explained by a pair
    (of the row or of a neighbour's SPFH) whose bin coordinate lies within
    1e-4 of a bin edge, where one ulp of acos / atan2 can move the pair to
    the next bin; those may be at most 0.5 % of the rows."""
    ok = np.isclose(got, want, rtol=1e-4, atol=1e-4).all(1)
    unexplained = np.nonzero(~ok & ~flagged)[0]
    assert unexplained.size == 0, (unexplained[:10],
                                   np.abs(got - want)[unexplained].max())
    assert (~ok).mean() <= 0.005, (~ok).mean()


MODES = [("hybrid", 100, 0.12), ("knn", 100, None), ("radius", None, 0.1)]


@pytest.mark.parametrize("mode,max_nn,radius", MODES)
def test_fpfh_float64_all_modes(mode, max_nn, radius):
    pts, nrm = _surface(3000, 1, np.float64)
    got = _reg().compute_fpfh_feature(_cuda(pts), _cuda(nrm), max_nn=max_nn,
                                      radius=radius).cpu().numpy()
    want = _oracle_full(pts, nrm, mode, max_nn, radius)
    assert got.shape == (3000, 33)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-4), \
        np.abs(got - want).max()
    assert (np.abs(got).sum(1) > 0).mean() > 0.99


@pytest.mark.parametrize("mode,max_nn,radius", MODES)
def test_fpfh_float32_all_modes(mode, max_nn, radius):
    pts, nrm = _surface(3000, 2, np.float32)
    got = _reg().compute_fpfh_feature(_cuda(pts), _cuda(nrm), max_nn=max_nn,
                                      radius=radius).cpu().numpy()
    want, flagged = _oracle_full(pts, nrm, mode, max_nn, radius,
                                 edge_tol=1e-4)
    _check_f32(got, want, flagged)


@pytest.mark.parametrize("max_nn", [100, 128])
def test_fpfh_max_nn_and_cap(max_nn):
    # lists beyond one wave (64): most are cut at max_nn
    pts, nrm = _surface(8000, 3, np.float64)
    got = _reg().compute_fpfh_feature(_cuda(pts), _cuda(nrm), max_nn=max_nn,
                                      radius=0.3).cpu().numpy()
    want = _oracle_full(pts, nrm, "hybrid", max_nn, 0.3)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-4)
    idx, _, cnt = orc.hybrid_search(pts, pts[:100], 0.3, max_nn)
    assert (cnt > 64).all() and (cnt == max_nn).mean() > 0.5
    from open3d_amd import _lib
    with pytest.raises(_lib.O3DMIError) as e:
        _reg().compute_fpfh_feature(_cuda(pts), _cuda(nrm), max_nn=129)
    assert e.value.status == 7  # O3DMI_ERR_UNSUPPORTED


@pytest.mark.parametrize("mode,max_nn,radius", MODES)
def test_fpfh_indices_subset_bit_identical(mode, max_nn, radius):
    pts, nrm = _surface(4000, 4, np.float32)
    P, N = _cuda(pts), _cuda(nrm)
    reg = _reg()
    full = reg.compute_fpfh_feature(P, N, max_nn=max_nn, radius=radius)
    full = full.cpu().numpy()
    idx = np.array([3999, 17, 5, 17, 2500, 0, 5, 1234], np.int64)
    sub = reg.compute_fpfh_feature(P, N, max_nn=max_nn, radius=radius,
                                   indices=idx).cpu().numpy()
    rows = np.unique(idx)
    assert sub.shape == (rows.size, 33)
    assert np.array_equal(sub, full[rows])
    empty = reg.compute_fpfh_feature(P, N, max_nn=max_nn, radius=radius,
                                     indices=np.zeros(0, np.int64))
    assert tuple(empty.shape) == (0, 33)


def test_fpfh_argument_errors():
    from open3d_amd import _lib
    pts, nrm = _surface(200, 5, np.float32)
    P, N = _cuda(pts), _cuda(nrm)
    reg = _reg()
    for kw in (dict(max_nn=3), dict(max_nn=None, radius=0.0),
               dict(max_nn=None, radius=-1.0), dict(max_nn=None, radius=None),
               dict(max_nn=10, indices=np.array([200], np.int64)),
               dict(max_nn=10, indices=np.array([-1], np.int64))):
        with pytest.raises(_lib.O3DMIError) as e:
            reg.compute_fpfh_feature(P, N, **kw)
        assert e.value.status == 1, kw  # O3DMI_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        reg.compute_fpfh_feature(P, None)
    L = _lib.lib()
    got = C.c_int64(0)
    out = torch.zeros((200, 33), dtype=torch.float32, device="cuda")
    st = L.o3dmi_registration_compute_fpfh_feature(
        _lib.ptr(P), None, 200, 0, 1, 30, 0, C.c_double(0), None, -1,
        _lib.ptr(out), C.byref(got), None)
    assert st == 1


def _features(n, dim, seed, dtype):
    rng = np.random.RandomState(seed)
    return rng.uniform(0, 1, (n, dim)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [33, 7])
def test_correspondences_exact(dtype, dim):
    src = _features(1500, dim, 10 + dim, dtype)
    tgt = _features(2300, dim, 20 + dim, dtype)
    # planted exact ties: two target rows equal to a source row; the lower
    # index must win
    tgt[700] = src[5]
    tgt[300] = src[5]
    tgt[1200] = src[9]
    tgt[1900] = src[9]
    # near-ties within 1e-6 relative
    tgt[50] = src[20] * (1 + 1e-6)
    tgt[40] = src[20] * (1 - 1e-6)
    got = _reg().correspondences_from_features(_cuda(src), _cuda(tgt))
    want, _ = fo.correspondences(src, tgt)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[5, 1] == 300 and want[9, 1] == 1200


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_correspondences_mutual_filter_both_outcomes(dtype):
    reg = _reg()
    # a permuted noisy copy: most pairs are mutual
    src = _features(3000, 33, 30, dtype)
    perm = np.random.RandomState(31).permutation(3000)
    tgt = (src[perm] + np.random.RandomState(32).normal(
        0, 1e-3, src.shape)).astype(dtype)
    got, fb = reg.correspondences_from_features(
        _cuda(src), _cuda(tgt), mutual_filter=True, return_fallback=True)
    want, wfb = fo.correspondences(src, tgt, mutual_filter=True)
    assert not fb and not wfb
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.shape[0] > 2900
    # unrelated sets: few mutual pairs -> fallback with the flag
    a = _features(2000, 33, 33, dtype)
    b = _features(500, 33, 34, dtype)
    got, fb = reg.correspondences_from_features(
        _cuda(a), _cuda(b), mutual_filter=True, mutual_consistency_ratio=0.5,
        return_fallback=True)
    want, wfb = fo.correspondences(a, b, mutual_filter=True, ratio=0.5)
    assert fb and wfb
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.shape[0] == 2000


def test_end_to_end_global_registration():
    """The tested pipeline: FPFH on a cloud and on a rigidly moved, permuted
    copy; mutual feature correspondences; of those, the pairs whose features
    agree to 1e-12 relative (the same neighbourhood, moved: neighbour lists
    that differ at the radius edge or a bin edge are dropped, as a RANSAC
    stage would drop them); Kabsch (o3dmi_compute_rt_p2point) recovers the
    motion."""
    from open3d_amd import _lib
    reg = _reg()
    rng = np.random.RandomState(40)
    pts, nrm0 = _surface(20000, 41, np.float64)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = 0.7
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    t = np.array([0.3, -0.2, 0.5])
    perm = rng.permutation(20000)
    src = pts[perm] @ R.T + t        # source = T * target, permuted
    src_hint = nrm0[perm] @ R.T
    P_t, P_s = _cuda(pts), _cuda(src)
    # normals from estimate_normals, oriented like the analytic ones
    n_t = reg.estimate_normals(P_t, max_nn=30, normals=_cuda(nrm0))
    n_s = reg.estimate_normals(P_s, max_nn=30, normals=_cuda(src_hint))
    f_t = reg.compute_fpfh_feature(P_t, n_t, max_nn=100, radius=0.1)
    f_s = reg.compute_fpfh_feature(P_s, n_s, max_nn=100, radius=0.1)
    corr = reg.correspondences_from_features(f_s, f_t, mutual_filter=True)
    c = corr.cpu().numpy()
    # keep the pairs whose features agree (the same neighbourhood, moved)
    fs, ft = f_s.cpu().numpy(), f_t.cpu().numpy()
    fd = ((fs[c[:, 0]] - ft[c[:, 1]]) ** 2).sum(1)
    c = c[fd <= 1e-12 * np.maximum((fs[c[:, 0]] ** 2).sum(1), 1.0)]
    assert c.shape[0] > 1000
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    from open3d_amd.core import stream
    # target -> source: R, t with source = R target + t
    inv = np.full(20000, -1, np.int64)
    inv[c[:, 1]] = c[:, 0]
    _lib.check(_lib.lib().o3dmi_icp_p2point_accumulate(
        _lib.ptr(P_t), _lib.ptr(P_s), _lib.ptr(_cuda(inv)), 20000, 1,
        _lib.ptr(sums), stream()), "p2point_accumulate")
    s = sums.cpu().numpy()
    Rg, tg = np.zeros(9), np.zeros(3)
    _lib.check(_lib.lib().o3dmi_compute_rt_p2point(
        _lib.f64p(s), _lib.f64p(Rg), _lib.f64p(tg)), "rt")
    Rg = Rg.reshape(3, 3)
    ang = np.arccos(np.clip((np.trace(Rg.T @ R) - 1) / 2, -1, 1))
    assert ang <= 1e-4, ang
    assert np.abs(tg - t).max() <= 1e-4, tg - t


def test_scale_fpfh_1m_and_correspondences_50k():
    reg = _reg()
    pts, nrm = _surface(1_000_000, 50, np.float32)
    P, N = _cuda(pts), _cuda(nrm)
    r = 0.02
    full = reg.compute_fpfh_feature(P, N, max_nn=100, radius=r)
    torch.cuda.synchronize()
    rows = np.sort(np.random.RandomState(51).choice(1_000_000, 2000, False))
    got = full[_cuda(rows)].cpu().numpy()
    # restatement on the sample: lists of the rows, then of their neighbours
    idx, d2, cnt = orc.hybrid_search(pts, pts[rows], r, 100)
    need = np.unique(np.concatenate([rows, idx[idx >= 0]]))
    li, ld, lc = orc.hybrid_search(pts, pts[need], r, 100)
    want, flagged = fo.fpfh_from_lists(pts, nrm, li, ld, counts=lc,
                                       edge_tol=1e-4, list_points=need,
                                       out_points=rows)
    _check_f32(got, want, flagged)

    a = _features(50000, 33, 52, np.float32)
    b = _features(50000, 33, 53, np.float32)
    corr = reg.correspondences_from_features(_cuda(a), _cuda(b))
    c = corr.cpu().numpy()
    sample = np.sort(np.random.RandomState(54).choice(50000, 2000, False))
    want = fo.nn1(a[sample], b)
    assert np.array_equal(c[sample, 1], want)
    assert np.array_equal(c[:, 0], np.arange(50000))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mutual", [False, True])
def test_correspondences_nan_and_inf_rows(dtype, mutual):
    """A source row with a NaN (all its distances NaN) or an inf feature gets
    an index in range: NaN counts as +inf, ties to the lowest index."""
    src = _features(700, 33, 60, dtype)
    tgt = _features(900, 33, 61, dtype)
    src[3, 7] = np.nan
    src[11, :] = np.nan
    src[20, 0] = np.inf
    tgt[5, 2] = np.nan
    got, fb = _reg().correspondences_from_features(
        _cuda(src), _cuda(tgt), mutual_filter=mutual, return_fallback=True)
    got = got.cpu().numpy()
    want, wfb = fo.correspondences(src, tgt, mutual_filter=mutual)
    assert fb == wfb
    assert np.array_equal(got, want)
    assert ((got[:, 1] >= 0) & (got[:, 1] < 900)).all()
    if not mutual:
        assert got[3, 1] == 0 and got[11, 1] == 0 and got[20, 1] == 0
