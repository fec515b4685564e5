"""RANSAC global registration on the MI355X, seam by seam and whole, against
the numpy restatement (tests/_ransac_oracle.py) and the pinned CPU body of
EvaluateRegistration (tests/_oracle.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _oracle as orc
import _ransac_oracle as ro
from test_feature_gpu import _cuda, _surface

pytestmark = pytest.mark.gpu

EDGE, DIST, NORMAL = ro.EDGE, ro.DISTANCE, ro.NORMAL


def _reg():
    from open3d_amd import registration
    return registration


def _lib():
    from open3d_amd import _lib
    return _lib


def _stream():
    from open3d_amd.core import stream
    return stream()


def _motion(seed, angle=0.7, t=(0.3, -0.2, 0.5)):
    rng = np.random.RandomState(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + \
        (1 - math.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def _pair(ns, nt, seed, dtype, noise=0.002):
    """Two different samplings of one surface; the target is the moved one:
    target = T source (+ noise), so T is the source-to-target motion."""
    src, sn = _surface(ns, seed, np.float64)
    tgt0, tn0 = _surface(nt, seed + 1000, np.float64)
    T = _motion(seed)
    rng = np.random.RandomState(seed + 7)
    tgt = tgt0 @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, tgt0.shape)
    return (src.astype(dtype), sn.astype(dtype), tgt.astype(dtype),
            (tn0 @ T[:3, :3].T).astype(dtype), T)


def _mixed_corres(src, tgt, T, n, outlier_share, seed):
    """n pairs: true nearest pairs (under T) and uniformly random ones."""
    rng = np.random.RandomState(seed)
    moved = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    rows = rng.randint(0, src.shape[0], n)
    idx, _, cnt = orc.hybrid_search(tgt.astype(np.float64), moved[rows], 0.2,
                                    1)
    near = idx.reshape(-1).astype(np.int64)
    rnd = rng.randint(0, tgt.shape[0], n)
    bad = (rng.uniform(size=n) < outlier_share) | (near < 0)
    return np.stack([rows, np.where(bad, rnd, near)], 1).astype(np.int64)


def _hypotheses(seed, first, count, src, tgt, corres, ransac_n=3, checkers=(),
                sn=None, tn=None, ns=None, nt=None):
    lib = _lib()
    dt = lib.F64 if src.dtype == torch.float64 else lib.F32
    smp = torch.full((count, ransac_n), -1, dtype=torch.int64, device="cuda")
    Ts = torch.zeros((count, 16), dtype=torch.float64, device="cuda")
    ps = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    types = (C.c_int * 3)(*([k for k, _ in checkers] + [0] * 3)[:3])
    thr = (C.c_double * 3)(*([t for _, t in checkers] + [0.0] * 3)[:3])
    st = lib.lib().o3dmi_ransac_hypotheses(
        C.c_uint64(seed), first, count, lib.ptr(src),
        src.shape[0] if ns is None else ns, lib.ptr(tgt),
        tgt.shape[0] if nt is None else nt, lib.ptr(sn), lib.ptr(tn), dt,
        lib.ptr(corres), corres.shape[0], ransac_n, len(checkers), types, thr,
        lib.ptr(smp), lib.ptr(Ts), lib.ptr(ps), _stream())
    lib.check(st, "ransac_hypotheses")
    torch.cuda.synchronize()
    return smp.cpu().numpy(), Ts.cpu().numpy(), ps.cpu().numpy()


class _Scorer:
    """o3dmi_ransac_score over one target index."""

    def __init__(self, src, tgt, corres, max_distance):
        lib = _lib()
        self.lib, self.src, self.tgt, self.corres = lib, src, tgt, corres
        self.h = C.c_void_p()
        dt = lib.F64 if src.dtype == torch.float64 else lib.F32
        lib.check(lib.lib().o3dmi_nns_create(
            lib.ptr(tgt), tgt.shape[0], dt, C.c_double(max_distance),
            _stream(), C.byref(self.h)), "nns_create")

    def __call__(self, Ts):
        lib = self.lib
        T = _cuda(np.ascontiguousarray(Ts, np.float64).reshape(-1, 16))
        b = T.shape[0]
        cnt = torch.full((b,), -1, dtype=torch.int64, device="cuda")
        cor = torch.full((b,), -1, dtype=torch.int64, device="cuda")
        d2 = torch.full((b,), -1.0, dtype=torch.float64, device="cuda")
        nbytes = lib.lib().o3dmi_ransac_score_scratch_bytes(
            self.src.shape[0], b)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64,
                              device="cuda")
        lib.check(lib.lib().o3dmi_ransac_score(
            self.h, lib.ptr(self.src), self.src.shape[0], lib.ptr(self.tgt),
            self.tgt.shape[0], lib.ptr(T), b, lib.ptr(self.corres),
            self.corres.shape[0], lib.ptr(cnt), lib.ptr(d2), lib.ptr(cor),
            lib.ptr(scratch), _stream()), "ransac_score")
        torch.cuda.synchronize()
        return cnt.cpu().numpy(), d2.cpu().numpy(), cor.cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        self.lib.lib().o3dmi_nns_destroy(self.h)


# ---- 1. samples -------------------------------------------------------------
@pytest.mark.parametrize("n_corres", [3, 1000, (1 << 20) + 7])
def test_samples_equal_oracle(n_corres):
    rng = np.random.RandomState(1)
    src, _ = _surface(500, 2, np.float32)
    tgt, _ = _surface(400, 3, np.float32)
    corres = np.stack([rng.randint(0, 500, n_corres),
                       rng.randint(0, 400, n_corres)], 1).astype(np.int64)
    S, Tg, Cg = _cuda(src), _cuda(tgt), _cuda(corres)
    for seed, first, n in [(0, 0, 3), (1, 5, 3), (2 ** 64 - 1, 777, 4),
                           (12345, (1 << 31) + 11, 3), (7, 1 << 40, 8)]:
        got, _, _ = _hypotheses(seed, first, 700, S, Tg, Cg, ransac_n=n)
        want = ro.samples(seed, first, 700, n, n_corres)
        assert np.array_equal(got, want), (seed, first, n)


# ---- 2. Kabsch and checks ---------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hypotheses_against_oracle(dtype):
    src, sn, tgt, tn, T = _pair(20000, 20000, 10, dtype)
    rng = np.random.RandomState(11)
    corres = np.stack([rng.randint(0, 20000, 5000),
                       rng.randint(0, 20000, 5000)], 1).astype(np.int64)
    # a tenth of them true pairs, so that every check has both outcomes
    corres[:500] = _mixed_corres(src, tgt, T, 500, 0.0, 12)
    checkers = [(EDGE, 0.9), (DIST, 0.08), (NORMAL, 0.5)]
    count = 20000
    smp, Ts, ps = _hypotheses(5, 0, count, _cuda(src), _cuda(tgt),
                              _cuda(corres), 3, checkers, _cuda(sn),
                              _cuda(tn))
    assert np.array_equal(smp, ro.samples(5, 0, count, 3, 5000))
    left_out = 0
    n_pass = 0
    for i in range(count):
        h = ro.hypothesis(src, tgt, corres, smp[i], checkers, sn, tn)
        if h["ratio"] > 1e-3:
            d = np.abs(Ts[i].reshape(4, 4) - h["T"]).max()
            assert d <= 1e-10, (i, d)
        if h["margin"] > 1e-9:
            assert bool(ps[i]) == h["passed"], (i, h)
            n_pass += h["passed"]
        if not (h["ratio"] > 1e-3 and h["margin"] > 1e-9):
            left_out += 1
    assert left_out <= 0.01 * count, left_out
    assert 0 < n_pass < count
    assert set(np.unique(ps)) <= {0, 1}


# ---- 3. scoring -------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scoring_exact(dtype):
    src, _, tgt, _, T = _pair(5003, 4801, 20, dtype)
    corres = _mixed_corres(src, tgt, T, 3001, 0.7, 21)
    r = 0.05
    S, Tg, Cg = _cuda(src), _cuda(tgt), _cuda(corres)
    smp, Th, _ = _hypotheses(3, 0, 250, S, Tg, Cg)
    far = np.eye(4)
    far[:3, 3] = [50, 0, 0]
    rng = np.random.RandomState(22)
    near = []
    for k in range(3):
        Tn = _motion(100 + k, 0.7 + 0.01 * rng.normal())
        near.append(Tn.reshape(16))
    Ts = np.concatenate([np.eye(4).reshape(1, 16), T.reshape(1, 16),
                         far.reshape(1, 16), np.array(near), Th], 0)
    assert Ts.shape[0] >= 256
    sc = _Scorer(S, Tg, Cg, r)
    try:
        cnt, d2, cor = sc(Ts)
        # bit-identical when repeated, whatever the chunking
        cnt2, d22, cor2 = sc(Ts[:77])
    finally:
        sc.close()
    assert np.array_equal(cnt[:77], cnt2) and np.array_equal(cor[:77], cor2)
    assert np.array_equal(d2[:77], d22)
    reg = _reg()
    some_inliers = 0
    for k in range(Ts.shape[0]):
        Tk = Ts[k].reshape(4, 4)
        e = orc.evaluate_registration(src, tgt, r, Tk)
        m = e["correspondences"] >= 0
        want_cnt = int(m.sum())
        assert cnt[k] == want_cnt, (k, cnt[k], want_cnt)
        # the matched d2 in the point dtype (the search's arithmetic), summed
        # in float64
        d = ro.move(src, Tk)[m] - tgt[e["correspondences"][m]]
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert dd.dtype == src.dtype
        want_sum = math.fsum(float(x) for x in dd)
        assert abs(d2[k] - want_sum) <= 1e-12 * want_sum, (k, d2[k], want_sum)
        assert cor[k] == ro.corres_inliers(src, tgt, corres, Tk, r), k
        some_inliers += want_cnt > 0
        # the same through o3dmi_registration_evaluate, one call per T
        g = reg.evaluate_registration(S, Tg, r, Tk)
        gc = int((g.correspondence_set >= 0).sum().item())
        assert cnt[k] == gc, (k, cnt[k], gc)
        assert g.fitness == (gc / src.shape[0] if gc else 0.0)
        assert abs(g.inlier_rmse ** 2 * gc - d2[k]) <= 1e-12 * d2[k], k
    assert cnt[0] >= 0 and cnt[1] > 0.5 * src.shape[0] and cnt[2] == 0
    assert cor[2] == 0 and cor[1] > 0.2 * corres.shape[0]
    assert some_inliers > 3


# ---- 4 / 5 / 8. the driver, replayed from the seams ---------------------------
def _replay(src, tgt, corres, r, ransac_n, checkers, max_iteration, confidence,
            seed, sn=None, tn=None):
    """The oracle's sequential loop fed with the device's own seam outputs
    over iterations 0 .. max_iteration."""
    S, Tg, Cg = _cuda(src), _cuda(tgt), _cuda(corres)
    SN = None if sn is None else _cuda(sn)
    TN = None if tn is None else _cuda(tn)
    ns, n = src.shape[0], corres.shape[0]
    _, Ts, ps = _hypotheses(seed, 0, max_iteration, S, Tg, Cg, ransac_n,
                            checkers, SN, TN)
    sc = _Scorer(S, Tg, Cg, r)
    cache = {}
    passing = np.nonzero(ps)[0]

    def score(i):
        if i not in cache:
            k = int(np.searchsorted(passing, i))
            rows = passing[k:k + 512]
            cnt, d2, cor = sc(Ts[rows])
            for j, row in enumerate(rows):
                cache[int(row)] = (int(cnt[j]), float(d2[j]), int(cor[j]))
        c, d, m = cache[i]
        f = c / ns if c else 0.0
        rm = math.sqrt(d / c) if c else 0.0
        return f, rm, m / n
    try:
        out = ro.loop(max_iteration, ransac_n, confidence,
                      lambda i: bool(ps[i]), score)
    finally:
        sc.close()
    b = out["best_iteration"]
    out["transformation"] = Ts[b].reshape(4, 4) if b >= 0 else np.eye(4)
    return out


def _run(src, tgt, corres, r, ransac_n=3, checkers=(), max_iteration=100000,
         confidence=0.999, seed=0, batch_size=0, sn=None, tn=None):
    reg = _reg()
    ch = []
    for kind, thr in checkers:
        ch.append({EDGE: reg.CorrespondenceCheckerBasedOnEdgeLength,
                   DIST: reg.CorrespondenceCheckerBasedOnDistance,
                   NORMAL: reg.CorrespondenceCheckerBasedOnNormal}[kind](thr))
    return reg.registration_ransac_based_on_correspondence(
        _cuda(src), _cuda(tgt), _cuda(corres), r, None, ransac_n, ch,
        reg.RANSACConvergenceCriteria(max_iteration, confidence), seed=seed,
        source_normals=None if sn is None else _cuda(sn),
        target_normals=None if tn is None else _cuda(tn),
        batch_size=batch_size)


def _same(got, want, src, tgt, r):
    assert got.best_iteration == want["best_iteration"]
    assert got.num_validations == want["num_validations"]
    assert got.final_iteration_bound == want["final_iteration_bound"]
    if want["best_iteration"] < 0:
        assert np.array_equal(got.transformation, np.eye(4))
        assert got.fitness == 0 and got.inlier_rmse == 0
        assert bool((got.correspondence_set == -1).all())
        return
    assert np.array_equal(got.transformation, want["transformation"])
    assert got.fitness == want["fitness"]
    # rule 7: the fields are the evaluate path's, bit for bit
    e = _reg().evaluate_registration(_cuda(src), _cuda(tgt), r,
                                     got.transformation)
    assert got.fitness == e.fitness and got.inlier_rmse == e.inlier_rmse
    assert np.array_equal(got.transformation, e.transformation)
    assert torch.equal(got.correspondence_set, e.correspondence_set)
    # the loop's own rmse: the same float64 terms summed in another order
    assert abs(got.inlier_rmse - want["inlier_rmse"]) <= \
        1e-12 * want["inlier_rmse"]


CASES = {
    # exits early: plenty of true pairs
    "early": dict(outliers=0.3, checkers=[(EDGE, 0.9), (DIST, 0.06)],
                  max_iteration=3000, confidence=0.999),
    # runs to max_iteration: mostly wrong pairs, few iterations
    "full": dict(outliers=0.9, checkers=[(EDGE, 0.9), (DIST, 0.06)],
                 max_iteration=1500, confidence=0.999),
    # every hypothesis fails the checks
    "none": dict(outliers=1.0, checkers=[(DIST, 1e-6)], max_iteration=1200,
                 confidence=0.999),
    # confidence 1.0 never exits
    "conf1": dict(outliers=0.3, checkers=[(EDGE, 0.9)], max_iteration=700,
                  confidence=1.0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_driver_equals_replay_for_every_batch_size(case):
    c = CASES[case]
    src, _, tgt, _, T = _pair(4000, 4100, 30, np.float32)
    corres = _mixed_corres(src, tgt, T, 3000, c["outliers"], 31)
    r = 0.04
    want = _replay(src, tgt, corres, r, 3, c["checkers"], c["max_iteration"],
                   c["confidence"], 9)
    if case == "early":
        assert want["final_iteration_bound"] < c["max_iteration"]
        assert want["best_iteration"] >= 0
    if case in ("full", "conf1"):
        assert want["final_iteration_bound"] == c["max_iteration"]
    if case == "conf1":
        assert want["best_iteration"] >= 0
    if case == "none":
        assert want["num_validations"] == 0
    for bs in (1, 64, 0):
        got = _run(src, tgt, corres, r, 3, c["checkers"], c["max_iteration"],
                   c["confidence"], 9, bs)
        _same(got, want, src, tgt, r)


def test_seeds_and_repeatability():
    src, _, tgt, _, T = _pair(4000, 4100, 40, np.float64)
    corres = _mixed_corres(src, tgt, T, 3000, 0.8, 41)
    kw = dict(checkers=[(EDGE, 0.9), (DIST, 0.06)], max_iteration=4000)
    a = _run(src, tgt, corres, 0.04, seed=1, **kw)
    b = _run(src, tgt, corres, 0.04, seed=1, batch_size=97, **kw)
    c = _run(src, tgt, corres, 0.04, seed=2, **kw)
    assert a.best_iteration >= 0 and c.best_iteration >= 0
    for f in ("best_iteration", "num_validations", "final_iteration_bound",
              "fitness", "inlier_rmse"):
        assert getattr(a, f) == getattr(b, f), f
    assert np.array_equal(a.transformation, b.transformation)
    assert torch.equal(a.correspondence_set, b.correspondence_set)
    assert a.best_iteration != c.best_iteration


# ---- 6. it registers things ---------------------------------------------------
def _pose_error(Tg, T):
    dR = Tg[:3, :3].T @ T[:3, :3]
    ang = math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1) / 2)))
    return ang, float(np.linalg.norm(Tg[:3, 3] - T[:3, 3]))


def _icp_from(src, tgt, tn, init):
    reg = _reg()
    return reg.multi_scale_icp(
        _cuda(src), _cuda(tgt), _cuda(tn), [-1.0],
        [reg.ICPConvergenceCriteria(1e-9, 1e-9, 50)], [0.03],
        init_source_to_target=init)


def test_registers_noisy_resampled_clouds():
    src, sn, tgt, tn, T = _pair(20000, 21000, 50, np.float32, noise=0.003)
    voxel = 0.03
    thr = 1.5 * voxel
    corres = _mixed_corres(src, tgt, T, 6000, 0.75, 51)
    got = _run(src, tgt, corres, thr, 3, [(EDGE, 0.9), (DIST, thr)], 100000,
               0.999, 3)
    assert got.best_iteration >= 0 and got.fitness > 0.5
    ang, dt = _pose_error(got.transformation, T)
    radius = float(np.linalg.norm(src, axis=1).max())
    assert ang <= thr / radius, ang
    assert dt <= thr, dt
    a = _icp_from(src, tgt, tn, got.transformation)
    b = _icp_from(src, tgt, tn, T)
    assert abs(a.fitness - b.fitness) <= 1e-3
    assert np.abs(a.transformation - b.transformation).max() <= 1e-3


def test_feature_matching_registers_down_sampled_clouds():
    reg = _reg()
    src, sn, tgt, tn, T = _pair(60000, 64000, 60, np.float32, noise=0.001)
    # _surface maps onto itself under a turn of 2 pi / 5 about z, and local
    # features cannot tell those five poses apart: both clouds lose the same
    # wedge of longitudes (no multiple of 2 pi / 5 wide), so that only the
    # true pose overlaps fully -- the partial overlap of real scans
    back = (tgt.astype(np.float64) - T[:3, 3]) @ T[:3, :3]
    keep_s = np.abs(np.arctan2(src[:, 1], src[:, 0]) - 0.1) > 0.6
    keep_t = np.abs(np.arctan2(back[:, 1], back[:, 0]) - 0.1) > 0.6
    src, sn, tgt, tn = src[keep_s], sn[keep_s], tgt[keep_t], tn[keep_t]
    voxel = 0.03
    thr = 1.5 * voxel
    ps, ns_ = reg.voxel_down_sample(_cuda(src), _cuda(sn), voxel)
    pt, nt_ = reg.voxel_down_sample(_cuda(tgt), _cuda(tn), voxel)
    fs = reg.compute_fpfh_feature(ps, ns_, max_nn=100, radius=5 * voxel)
    ft = reg.compute_fpfh_feature(pt, nt_, max_nn=100, radius=5 * voxel)
    got = reg.registration_ransac_based_on_feature_matching(
        ps, pt, fs, ft, True, thr, None, 3,
        [reg.CorrespondenceCheckerBasedOnEdgeLength(0.9),
         reg.CorrespondenceCheckerBasedOnDistance(thr)],
        reg.RANSACConvergenceCriteria(100000, 0.999), seed=4)
    assert got.best_iteration >= 0
    ang, dt = _pose_error(got.transformation, T)
    radius = float(ps.norm(dim=1).max().item())
    assert ang <= thr / radius, ang
    assert dt <= thr, dt
    # the same call in two steps
    corres = reg.correspondences_from_features(fs, ft, mutual_filter=True)
    two = reg.registration_ransac_based_on_correspondence(
        ps, pt, corres, thr, None, 3,
        [reg.CorrespondenceCheckerBasedOnEdgeLength(0.9),
         reg.CorrespondenceCheckerBasedOnDistance(thr)],
        reg.RANSACConvergenceCriteria(100000, 0.999), seed=4)
    assert two.best_iteration == got.best_iteration
    assert np.array_equal(two.transformation, got.transformation)
    P, Q, N = ps.cpu().numpy(), pt.cpu().numpy(), nt_.cpu().numpy()
    a = _icp_from(P, Q, N, got.transformation)
    b = _icp_from(P, Q, N, T)
    assert abs(a.fitness - b.fitness) <= 1e-3
    assert np.abs(a.transformation - b.transformation).max() <= 1e-3


# ---- 7. errors and edges ------------------------------------------------------
def test_errors_and_edges():
    reg, lib = _reg(), _lib()
    src, sn, tgt, tn, T = _pair(1500, 1600, 70, np.float32)
    corres = _mixed_corres(src, tgt, T, 800, 0.5, 71)
    S, Tg, Cg = _cuda(src), _cuda(tgt), _cuda(corres)
    crit = reg.RANSACConvergenceCriteria(500, 0.999)

    def empty(res):
        return (np.array_equal(res.transformation, np.eye(4)) and
                res.fitness == 0 and res.inlier_rmse == 0 and
                res.best_iteration == -1 and res.num_validations == 0)
    f = reg.registration_ransac_based_on_correspondence
    assert empty(f(S, Tg, Cg, 0.05, None, 2, [], crit))
    assert empty(f(S, Tg, Cg[:2], 0.05, None, 3, [], crit))
    assert empty(f(S, Tg, Cg, 0.0, None, 3, [], crit))
    assert empty(f(S, Tg, Cg, -1.0, None, 3, [], crit))
    for est, n in ((reg.TransformationEstimationPointToPlane(), 3),
                   (reg.TransformationEstimationPointToPoint(True), 3),
                   (None, 9)):
        with pytest.raises(lib.O3DMIError) as e:
            f(S, Tg, Cg, 0.05, est, n, [], crit)
        assert e.value.status == 7  # O3DMI_ERR_UNSUPPORTED
    for row in ([1500, 0], [0, 1600], [-1, 0]):
        bad = corres.copy()
        bad[400] = row
        with pytest.raises(lib.O3DMIError) as e:
            f(S, Tg, _cuda(bad), 0.05, None, 3, [], crit)
        assert e.value.status == 1  # O3DMI_ERR_INVALID_ARG
    # zero checkers: every non-degenerate sample is validated
    want = _replay(src, tgt, corres, 0.05, 3, [], 500, 0.999, 0)
    got = f(S, Tg, Cg, 0.05, None, 3, [], crit)
    _same(got, want, src, tgt, 0.05)
    assert got.num_validations > 0
    # ransac_n = 8
    want = _replay(src, tgt, corres, 0.05, 8, [(EDGE, 0.8)], 500, 0.999, 0)
    got = f(S, Tg, Cg, 0.05, None, 8,
            [reg.CorrespondenceCheckerBasedOnEdgeLength(0.8)], crit)
    _same(got, want, src, tgt, 0.05)
    # the normal checker without normals passes everything; with them it
    # rejects some
    ch = [reg.CorrespondenceCheckerBasedOnNormal(0.3)]
    without = f(S, Tg, Cg, 0.05, None, 3, ch, crit)
    assert without.num_validations == got_validations(src, tgt, corres)
    with_n = f(S, Tg, Cg, 0.05, None, 3, ch, crit, source_normals=_cuda(sn),
               target_normals=_cuda(tn))
    want = _replay(src, tgt, corres, 0.05, 3, [(NORMAL, 0.3)], 500, 0.999, 0,
                   sn, tn)
    _same(with_n, want, src, tgt, 0.05)
    # the same kind twice
    with pytest.raises(lib.O3DMIError) as e:
        f(S, Tg, Cg, 0.05, None, 3, ch + ch, crit)
    assert e.value.status == 1


def got_validations(src, tgt, corres):
    return _replay(src, tgt, corres, 0.05, 3, [], 500, 0.999, 0)[
        "num_validations"]


# ---- 8. scale -----------------------------------------------------------------
def test_scale_100k_iterations():
    src, _, tgt, _, T = _pair(20000, 20500, 80, np.float32, noise=0.003)
    # most pairs wrong and confidence 1.0: all 100 000 iterations run
    corres = _mixed_corres(src, tgt, T, 20000, 0.92, 81)
    r = 0.045
    checkers = [(EDGE, 0.9), (DIST, r)]
    got = _run(src, tgt, corres, r, 3, checkers, 100000, 1.0, 5)
    assert got.final_iteration_bound == 100000
    assert got.iterations_run == 100000
    # past the first rounds the batch has grown to its cap
    assert got.num_batches < 100000 // 1024
    # the replay over all 100 000 iterations, exact
    want = _replay(src, tgt, corres, r, 3, checkers, 100000, 1.0, 5)
    assert want["num_validations"] > 0 and want["best_iteration"] >= 0
    _same(got, want, src, tgt, r)
    # and at upstream's confidence: the bound falls several rounds into the run
    got = _run(src, tgt, corres, r, 3, checkers, 100000, 0.999, 5)
    want = _replay(src, tgt, corres, r, 3, checkers, 100000, 0.999, 5)
    _same(got, want, src, tgt, r)
