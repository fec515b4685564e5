"""Fast Global Registration on the MI355X, seam by seam and whole, against the
numpy restatement (tests/_fgr_oracle.py).

The tuple test is bit exact against the restatement. The optimisation differs
from it only in sin / cos / sqrt / divide rounding over the iterations; its pass
mark is the project's pose tolerance (README: 1e-6 rad / 1e-5 m) applied to the
Frobenius and translation differences on scenes of unit scale. The two forms of
the optimisation (resident, streamed) must return the same bits."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _fgr_oracle as fo

pytestmark = pytest.mark.gpu

TOL_ROT, TOL_T = 1e-6, 1e-5      # the project's pose tolerance
BOUND_RAD, BOUND_T = 5e-3, 5e-3  # ground truth, as tests/test_fgr_cpu.py
RESIDENT, STREAMED = 1, 2
INVALID_ARG = 1


def _L():
    from open3d_amd import _lib
    return _lib


def _reg():
    from open3d_amd import registration
    return registration


def _stream():
    from open3d_amd.core import stream
    return stream()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _scene(n, share, seed, n_corres=None):
    return fo.scene(n, share, seed, n_corres=n_corres)


# ---- the tuple seam -----------------------------------------------------------
def _tuple(src, tgt, corres, scale, cap, seed, first_batch=None):
    L = _L()
    dt = L.F64 if src.dtype == np.float64 else L.F32
    n = corres.shape[0]
    rows = 3 * min(cap, 100 * n)
    out = torch.full((max(rows, 1), 2), -7, dtype=torch.int64, device="cuda")
    nt, ntr, nb = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    s, t, c = _cuda(src), _cuda(tgt), _cuda(corres)
    if first_batch is None:
        st = L.lib().o3dmi_fgr_tuple_test(
            C.c_uint64(seed), L.ptr(s), s.shape[0], L.ptr(t), t.shape[0], dt,
            L.ptr(c), n, C.c_double(scale), cap, L.ptr(out), C.byref(nt),
            C.byref(ntr), _stream())
    else:
        st = L.lib().o3dmi_internal_fgr_tuple_test(
            C.c_uint64(seed), L.ptr(s), s.shape[0], L.ptr(t), t.shape[0], dt,
            L.ptr(c), n, C.c_double(scale), cap, first_batch, L.ptr(out),
            C.byref(nt), C.byref(ntr), C.byref(nb), _stream())
    L.check(st, "fgr_tuple_test")
    torch.cuda.synchronize()
    return out.cpu().numpy(), nt.value, ntr.value, nb.value


def _check_tuple(src, tgt, corres, scale, cap, seed, first_batch=None):
    want, n_want, trials_want = fo.tuple_test(src, tgt, corres, scale, cap,
                                              seed)
    got, n, trials, batches = _tuple(src, tgt, corres, scale, cap, seed,
                                     first_batch)
    assert (n, trials) == (n_want, trials_want)
    assert np.array_equal(got[:3 * n], want)
    assert (got[3 * n:] == -7).all()  # nothing past the kept tuples
    return n, trials, batches


@pytest.mark.parametrize("share,seed", [(0.5, 1), (0.7, 2)])
def test_tuple_seam_matches_the_restatement(share, seed):
    src, tgt, corres, _ = _scene(300, share, seed)
    n, trials, _ = _check_tuple(src, tgt, corres, 0.95, 1000, seed)
    if share == 0.5:
        assert n == 1000 and trials < 30000   # stops early at the cap
    else:
        assert n < 1000 and trials == 30000   # runs every trial
    # Float32 points are widened on load
    _check_tuple(src.astype(np.float32), tgt.astype(np.float32), corres, 0.95,
                 1000, seed)


def test_tuple_seam_cap_inside_a_later_batch():
    src, tgt, corres, _ = _scene(300, 0.5, 1)
    # batches of 256, 512, 1024, ...: the cap of 1000 tuples falls at trial
    # ~9000, inside the sixth batch
    n, trials, batches = _check_tuple(src, tgt, corres, 0.95, 1000, 1,
                                      first_batch=256)
    assert n == 1000 and batches >= 5
    done = 256 * (2 ** batches - 1)
    assert done >= trials > 256 * (2 ** (batches - 1) - 1)
    # the same tuples whatever the first batch
    a = _tuple(src, tgt, corres, 0.95, 1000, 1, first_batch=1000)
    b = _tuple(src, tgt, corres, 0.95, 1000, 1)
    assert np.array_equal(a[0], b[0]) and a[1:3] == b[1:3]


def test_tuple_seam_caps_and_small_sets():
    src, tgt, corres, _ = _scene(300, 0.5, 1)
    n, trials, _ = _check_tuple(src, tgt, corres, 0.95, 1, 3)
    assert n == 1
    # a cap no input reaches
    n, trials, _ = _check_tuple(src, tgt, corres, 0.95, 10 ** 6, 3)
    assert 1000 < n < 10 ** 6 and trials == 30000
    # ncorr = 3: 300 trials over three pairs; <= 2: nothing
    _check_tuple(src, tgt, corres[:3], 0.95, 1000, 0)
    true = corres[np.linalg.norm(
        src[corres[:, 0]] @ _scene(300, 0.5, 1)[3][:3, :3].T +
        _scene(300, 0.5, 1)[3][:3, 3] - tgt[corres[:, 1]], axis=1) < 0.02][:3]
    n, _, _ = _check_tuple(src, tgt, true, 0.95, 1000, 0)
    assert n > 0  # three true pairs: the trials with distinct draws pass
    for m in (0, 1, 2):
        got, n, trials, _ = _tuple(src, tgt, corres[:m].reshape(-1, 2), 0.95,
                                   1000, 0)
        assert n == 0 and trials == 0 and (got == -7).all()


# ---- the optimise seam ----------------------------------------------------------
def _optimize(src, tgt, corres, par, form, division_factor=1.4,
              decrease_mu=True, max_dist=0.025, iterations=64):
    L = _L()
    n = corres.shape[0]
    out = torch.full((18,), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = L.lib().o3dmi_internal_fgr_stream_scratch_bytes(n)
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    s, t, c = _cuda(src), _cuda(tgt), _cuda(corres)
    ran = C.c_int(-1)
    st = L.lib().o3dmi_internal_fgr_optimize(
        L.ptr(s), s.shape[0], L.ptr(t), t.shape[0], L.ptr(c), n,
        C.c_double(par), C.c_double(division_factor), int(decrease_mu),
        C.c_double(max_dist), iterations, form, L.ptr(scratch), L.ptr(out),
        C.byref(ran), _stream())
    L.check(st, "fgr_optimize")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:16].reshape(4, 4).copy(), float(o[16]), int(o[17]), ran.value


@functools.lru_cache(maxsize=None)
def _normalised(n_corres):
    """Pairs drawn (with repeats) from the 1000-point scene at 50 % random,
    on the normalised clouds: unit scale."""
    src, tgt, corres, T = _scene(1000, 0.5, 4, n_corres)
    nrm = fo.normalize(src, tgt)
    return nrm["clouds"][0], nrm["clouds"][1], corres, nrm["scale_global"]


def _capacity():
    return _L().lib().o3dmi_internal_fgr_resident_capacity()


@pytest.mark.parametrize("count", [10, 255, 256, 257, 3000, "capacity+1"])
def test_optimize_forms_agree_and_match_the_restatement(count):
    cap = _capacity()
    assert cap == 4096
    n = cap + 1 if count == "capacity+1" else count
    src, tgt, corres, par = _normalised(n)
    want, want_par, want_failed = fo.optimize(src, tgt, corres, par)
    forms = [STREAMED] if n > cap else [RESIDENT, STREAMED]
    got = {f: _optimize(src, tgt, corres, par, f) for f in forms}
    for f in forms:
        T, fpar, failed, ran = got[f]
        assert ran == f and failed == want_failed == 0
        assert fpar == want_par  # divisions only: correctly rounded
        rot, tr = fo.pose_change(T, want)
        print("count %d form %d: device - restatement %.2e (Frobenius) / "
              "%.2e (translation)" % (n, f, rot, tr))
        assert rot < TOL_ROT and tr < TOL_T
        assert np.array_equal(T[3], [0, 0, 0, 1])
    if len(forms) == 2:
        assert got[RESIDENT][0].tobytes() == got[STREAMED][0].tobytes()
        assert got[RESIDENT][1:3] == got[STREAMED][1:3]
    # the automatic choice
    auto = _optimize(src, tgt, corres, par, 0)
    assert auto[3] == (STREAMED if n > cap else RESIDENT)
    assert auto[0].tobytes() == got[forms[-1]][0].tobytes()
    if n > cap:
        L = _L()
        assert L.lib().o3dmi_fgr_optimize_scratch_bytes(n) == \
            L.lib().o3dmi_internal_fgr_stream_scratch_bytes(n) > 0
        # the resident form refuses what it cannot hold
        with pytest.raises(L.O3DMIError):
            _optimize(src, tgt, corres, par, RESIDENT)


@pytest.mark.parametrize("kw", [dict(decrease_mu=False),
                                dict(iterations=0), dict(iterations=1),
                                dict(par=2.5, division_factor=1.1,
                                     max_dist=0.3)])
def test_optimize_options(kw):
    src, tgt, corres, par = _normalised(700)
    kw = dict(kw)
    par = kw.pop("par", par)
    want, want_par, want_failed = fo.optimize(
        src, tgt, corres, par, kw.get("division_factor", 1.4),
        kw.get("decrease_mu", True), kw.get("max_dist", 0.025),
        kw.get("iterations", 64))
    a = _optimize(src, tgt, corres, par, RESIDENT, **kw)
    b = _optimize(src, tgt, corres, par, STREAMED, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1:3] == b[1:3]
    assert a[1] == want_par and a[2] == want_failed
    rot, tr = fo.pose_change(a[0], want)
    assert rot < TOL_ROT and tr < TOL_T
    if kw.get("iterations") == 0:
        assert np.array_equal(a[0], np.eye(4)) and a[1] == par and a[3] == 0
    if kw.get("decrease_mu") is False:
        assert a[1] == par


def test_optimize_fewer_than_ten_and_degenerate():
    src, tgt, corres, par = _normalised(700)
    T, fpar, failed, ran = _optimize(src, tgt, corres[:9], par, 0)
    assert np.array_equal(T, np.eye(4)) and fpar == par and failed == 0
    assert ran == 0
    # all pairs one point on the z axis, p == q: s = 1, JTJ = 64 x an integer
    # matrix of rank 3, exactly: its third pivot is 0 in every iteration
    p = np.tile([[0.0, 0.0, 1.0]], (4, 1))
    pairs = np.zeros((64, 2), np.int64)
    for form in (RESIDENT, STREAMED):
        T, fpar, failed, ran = _optimize(p, p, pairs, 1.0, form, iterations=7)
        assert failed == 7 and ran == form
        assert np.isfinite(T).all() and np.array_equal(T, np.eye(4))
        assert np.isfinite(fpar)
    assert fo.optimize(p, p, pairs, 1.0, iteration_number=7)[2] == 7
    # a pair outside the clouds is never read and adds zeros
    bad = corres[:300].copy()
    bad[5] = [10 ** 9, 0]
    bad[17] = [0, -1]
    keep = np.ones(300, bool)
    keep[[5, 17]] = False
    a = _optimize(src, tgt, bad, par, RESIDENT)
    b = _optimize(src, tgt, bad, par, STREAMED)
    assert a[0].tobytes() == b[0].tobytes()
    assert np.isfinite(a[0]).all()


# ---- whole calls ------------------------------------------------------------------
def _option(**kw):
    return _reg().FastGlobalRegistrationOption(**kw)


def _check_result(res, src_t, tgt_t, max_dist):
    """Rule 5: result = evaluate on the returned transformation, bit for bit."""
    ev = _reg().evaluate_registration(src_t, tgt_t, max_dist,
                                      res.transformation)
    assert res.fitness == ev.fitness and res.inlier_rmse == ev.inlier_rmse
    assert torch.equal(res.correspondence_set, ev.correspondence_set)
    assert res.fitness > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("tuple_test", [True, False])
def test_whole_call_on_correspondences(dtype, tuple_test):
    src, tgt, corres, T = _scene(300, 0.5, 1)
    src, tgt = src.astype(dtype), tgt.astype(dtype)
    s, t, c = _cuda(src), _cuda(tgt), _cuda(corres)
    res, info = _reg().registration_fgr_based_on_correspondence(
        s, t, c, _option(tuple_test=tuple_test, seed=1))
    _check_result(res, s, t, 0.025)
    want, winfo = fo.fgr_correspondence(src, tgt, corres,
                                        tuple_test=tuple_test, seed=1)
    assert info["n_initial"] == 300 and info["swapped"] == 0
    assert info["n_tuples"] == winfo["n_tuples"]
    assert info["n_trials"] == winfo["n_trials"]
    assert info["n_used"] == winfo["n_used"] == (3000 if tuple_test else 300)
    assert info["form"] == RESIDENT and info["failed_solves"] == 0
    assert abs(info["scale_global"] - winfo["scale_global"]) < 1e-14
    assert abs(info["final_par"] - winfo["final_par"]) < 1e-14
    rot, tr = fo.pose_change(res.transformation, want)
    print("whole call: device - restatement %.2e / %.2e" % (rot, tr))
    assert rot < TOL_ROT and tr < TOL_T
    ang, dist = fo.pose_error(res.transformation, T)
    assert ang < BOUND_RAD and dist < BOUND_T


def test_whole_call_absolute_scale_and_identity_paths():
    src, tgt, corres, T = _scene(300, 0.5, 1)
    s, t, c = _cuda(src), _cuda(tgt), _cuda(corres)
    reg = _reg()
    # use_absolute_scale: scale_global = 1, and par starts there (rule 4)
    opt = dict(tuple_test=False, use_absolute_scale=True,
               maximum_correspondence_distance=0.03)
    res, info = reg.registration_fgr_based_on_correspondence(
        s, t, c, _option(**opt))
    want, winfo = fo.fgr_correspondence(src, tgt, corres, **opt)
    assert info["scale_global"] == 1.0 == winfo["scale_global"]
    assert info["final_par"] == winfo["final_par"]
    rot, tr = fo.pose_change(res.transformation, want)
    assert rot < TOL_ROT and tr < TOL_T
    _check_result(res, s, t, 0.03)
    # 9 pairs, and no iteration: rule 5 on the identity (the mean shift)
    shift = np.eye(4)
    shift[:3, 3] = -(fo.sum_levels(src) / 300.0 - fo.sum_levels(tgt) / 300.0)
    for pairs, o in ((c[:9], dict(tuple_test=False)),
                     (c, dict(tuple_test=False, iteration_number=0)),
                     (c[:2], dict(tuple_test=True))):
        res, info = reg.registration_fgr_based_on_correspondence(
            s, t, pairs, _option(**o))
        assert np.array_equal(res.transformation, shift)
        assert info["form"] == 0 and info["failed_solves"] == 0
        ev = reg.evaluate_registration(s, t, 0.025, shift)
        assert (res.fitness, res.inlier_rmse) == (ev.fitness, ev.inlier_rmse)


def test_whole_call_refusals_write_nothing():
    L = _L()
    src, tgt, corres, _ = _scene(300, 0.5, 1)
    s, t = _cuda(src), _cuda(tgt)

    def call(pairs, cloud=s, **kw):
        opt = L.FgrOptionsC(1.4, 0, 1, 0.025, 64, 0.95, 1000, 1, 0)
        for k, v in kw.items():
            setattr(opt, k, v)
        c = _cuda(pairs)
        corr = torch.full((300,), -5, dtype=torch.int64, device="cuda")
        res = L.RegistrationResultC()
        res.fitness = -3.0
        res.inlier_rmse = -4.0
        info = L.FgrInfoC()
        info.n_used = -9
        st = L.lib().o3dmi_registration_fgr_correspondence(
            L.ptr(cloud), 300, L.ptr(t), 300, L.F64, L.ptr(c), c.shape[0],
            C.byref(opt), L.ptr(corr), C.byref(res), C.byref(info),
            _stream())
        torch.cuda.synchronize()
        untouched = (res.fitness == -3.0 and res.inlier_rmse == -4.0 and
                     info.n_used == -9 and bool((corr == -5).all()))
        return st, untouched

    assert call(corres)[0] == 0
    for kw in (dict(maximum_tuple_count=0), dict(maximum_tuple_count=-1),
               dict(division_factor=0.0), dict(division_factor=math.nan),
               dict(tuple_scale=math.inf), dict(tuple_scale=-0.95),
               dict(maximum_correspondence_distance=0.0),
               dict(maximum_correspondence_distance=math.inf),
               dict(iteration_number=-1)):
        assert call(corres, **kw) == (INVALID_ARG, True), kw
    for row in ([300, 0], [0, 300], [-1, 5], [5, -1]):
        bad = corres.copy()
        bad[123] = row
        assert call(bad) == (INVALID_ARG, True), row
        assert call(bad, tuple_test=0) == (INVALID_ARG, True), row
    # the finiteness gate
    nan = src.copy()
    nan[77, 1] = np.nan
    assert call(corres, cloud=_cuda(nan)) == (INVALID_ARG, True)
    # scale_global <= 0: both clouds one point (the origin: its sums are exact)
    one = np.zeros((300, 3))
    L2 = L.lib().o3dmi_registration_fgr_correspondence
    opt = L.FgrOptionsC(1.4, 0, 1, 0.025, 64, 0.95, 1000, 0, 0)
    res = L.RegistrationResultC()
    o, c = _cuda(one), _cuda(corres)
    assert L2(L.ptr(o), 300, L.ptr(o), 300, L.F64, L.ptr(c), 300,
              C.byref(opt), None, C.byref(res), None,
              _stream()) == INVALID_ARG


# ---- the feature entry point ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _feature_scene(ns, nt, seed):
    """min(ns, nt) true matches: the smaller cloud is a moved, shuffled part
    of the larger one. 33-D Float32 features: random rows; the target rows of
    true matches are the source rows plus small noise, the rest fresh random
    rows."""
    rng = np.random.RandomState(seed)
    big, small = max(ns, nt), min(ns, nt)
    src_all, _, _, T = fo.scene(big, 0.0, seed)
    moved = src_all @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.002, (big, 3))
    pick = rng.permutation(big)[:small]
    if ns >= nt:
        src, tgt = src_all, moved[pick]
        match_s, match_t = pick, np.arange(small)
    else:
        src, tgt = src_all[pick], moved
        match_s, match_t = np.arange(small), pick
    fs = rng.uniform(0, 1, (ns, 33)).astype(np.float32)
    ft = rng.uniform(0, 1, (nt, 33)).astype(np.float32)
    ft[match_t] = fs[match_s] + rng.normal(0, 0.01, (small, 33)).astype(
        np.float32)
    # a fifth of the matches get fresh random features: wrong pairs remain
    spoil = match_t[rng.uniform(size=small) < 0.2]
    ft[spoil] = rng.uniform(0, 1, (len(spoil), 33)).astype(np.float32)
    return src, tgt, fs, ft, T


def test_feature_nn1_seam_matches_its_definition():
    L = _L()
    _, _, fs, ft, _ = _feature_scene(400, 300, 5)
    a, b = _cuda(fs), _cuda(ft)
    nn = torch.full((400,), -1, dtype=torch.int32, device="cuda")
    L.check(L.lib().o3dmi_internal_feature_nn1(
        L.ptr(a), 400, L.ptr(b), 300, 33, L.F32, L.ptr(nn), _stream()),
        "feature_nn1")
    torch.cuda.synchronize()
    assert np.array_equal(nn.cpu().numpy(), fo.nn1(fs, ft))


@pytest.mark.parametrize("ns,nt", [(400, 300), (300, 400)])
def test_whole_call_on_features(ns, nt):
    src, tgt, fs, ft, T = _feature_scene(ns, nt, 5)
    s, t, a, b = _cuda(src), _cuda(tgt), _cuda(fs), _cuda(ft)
    reg = _reg()
    res, info = reg.registration_fgr_based_on_feature_matching(
        s, t, a, b, _option(seed=9))
    want, winfo = fo.fgr_feature_matching(src, tgt, fs, ft, seed=9)
    # rule 6: the larger cloud is the query side
    assert info["swapped"] == winfo["swapped"] == (1 if ns < nt else 0)
    assert info["n_initial"] == winfo["n_initial"] > 100
    assert info["n_tuples"] == winfo["n_tuples"] > 0
    assert info["n_trials"] == winfo["n_trials"]
    assert info["n_used"] == winfo["n_used"]
    rot, tr = fo.pose_change(res.transformation, want)
    assert rot < TOL_ROT and tr < TOL_T
    ang, dist = fo.pose_error(res.transformation, T)
    assert ang < BOUND_RAD and dist < BOUND_T
    _check_result(res, s, t, 0.025)
    # without the tuple test the source is the query side, and the call is
    # the correspondence call on the cross-checked pairs, bit for bit
    off = _option(tuple_test=False)
    res0, info0 = reg.registration_fgr_based_on_feature_matching(s, t, a, b,
                                                                 off)
    pairs = fo.initial_matching(fs, ft)
    assert info0["swapped"] == 0 and info0["n_initial"] == len(pairs)
    assert info0["n_used"] == len(pairs) and info0["n_tuples"] == 0
    res1, info1 = reg.registration_fgr_based_on_correspondence(
        s, t, _cuda(pairs), off)
    assert res0.transformation.tobytes() == res1.transformation.tobytes()
    assert (res0.fitness, res0.inlier_rmse) == (res1.fitness,
                                                res1.inlier_rmse)
    assert torch.equal(res0.correspondence_set, res1.correspondence_set)
    assert info0["final_par"] == info1["final_par"]


def test_repeatability():
    src, tgt, corres, _ = _scene(300, 0.7, 2)
    s, t, c = _cuda(src.astype(np.float32)), _cuda(tgt.astype(np.float32)), \
        _cuda(corres)
    runs = [_reg().registration_fgr_based_on_correspondence(
        s, t, c, _option(seed=2)) for _ in range(2)]
    (r0, i0), (r1, i1) = runs
    assert r0.transformation.tobytes() == r1.transformation.tobytes()
    assert (r0.fitness, r0.inlier_rmse) == (r1.fitness, r1.inlier_rmse)
    assert torch.equal(r0.correspondence_set, r1.correspondence_set)
    assert i0 == i1
