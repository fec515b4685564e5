"""Doppler ICP (TransformationEstimationForDopplerICP) on the GPU against the
numpy oracle of _doppler_oracle.py: the accumulate kernel, the host
preparation, the pyramid's 1-column attribute, the driver."""
import ctypes as C

import numpy as np
import pytest
import torch

import _doppler_oracle as dop
import _oracle as orc
from test_oracle_goldens import CORR, SRC, TGT, TGT_N

pytestmark = pytest.mark.gpu

INVALID_ARG, SINGULAR, UNSUPPORTED = 1, 5, 7


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib, registration
    return _lib, registration


def _pose_err(Ta, Tb):
    d = np.linalg.inv(Ta) @ Tb
    skew = d[:3, :3] - d[:3, :3].T
    ang = float(np.linalg.norm([skew[2, 1], skew[0, 2], skew[1, 0]]) / 2)
    return ang, float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))


def _f64p(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(
        C.POINTER(C.c_double))


def _accumulate(_lib, dev, n, nt, prep, period, reject, threshold, kg, kd,
                lam, sums):
    """o3dmi_icp_doppler_accumulate on device tensors dev = (src, dopplers,
    directions, tgt, tgt_normals, corr) -> status."""
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    R, r, w, v = (np.asarray(a, np.float64) for a in prep)
    return _lib.lib().o3dmi_icp_doppler_accumulate(
        *[_lib.ptr(t) for t in dev], n, nt, TORCH_TO_O3DMI[dev[0].dtype],
        _f64p(R), _f64p(r), _f64p(w), _f64p(v), C.c_double(period),
        int(reject), C.c_double(threshold), kg[0], C.c_double(kg[1]),
        C.c_double(kg[2]), kd[0], C.c_double(kd[1]), C.c_double(kd[2]),
        C.c_double(lam), _lib.ptr(sums), stream())


V_LEVER = np.array([[0.0, -1.0, 0.0, 0.4], [1.0, 0.0, 0.0, -0.2],
                    [0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0]])


def _accumulate_case(n, dtype, seed=0):
    """n source rows against 3 n / 4 + 5 target points, ~20 % of rows -1, the
    pairs a few centimetres apart; a lever arm so that every Jacobian column
    is exercised."""
    rng = np.random.default_rng(seed + n)
    nt = 3 * n // 4 + 5
    tgt = rng.uniform(-3, 3, (nt, 3))
    tn = rng.standard_normal((nt, 3))
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    corr = rng.integers(0, nt, n).astype(np.int64)
    src = tgt[corr] + 0.05 * rng.standard_normal((n, 3))
    corr[rng.random(n) < 0.2] = -1
    if n == 1:
        corr[0] = nt - 1
    dirs = src / np.linalg.norm(src, axis=1, keepdims=True)
    T = orc.pose_to_transformation([0.02, -0.03, 0.01, 0.1, -0.05, 0.07])
    prep = dop.host_prepare(V_LEVER, T, 0.1, dtype)
    dops = dop.predicted_doppler(dirs.astype(dtype), *prep)
    dops = dops + (0.3 * rng.standard_normal(n)).astype(dtype)
    arrays = [np.ascontiguousarray(a.astype(dtype))
              for a in (src, dops, dirs, tgt, tn)] + [corr]
    return arrays, nt, prep


SETTINGS = {
    "l2_l2": dict(kg=(0, 1.0, 1.0), kd=(0, 1.0, 1.0), reject=False),
    "huber_l2": dict(kg=(dop.HUBER, 0.03, 1.0), kd=(0, 1.0, 1.0),
                     reject=False),
    "l2_tukey": dict(kg=(0, 1.0, 1.0), kd=(dop.TUKEY, 0.05, 1.0),
                     reject=False),
    "reject": dict(kg=(dop.CAUCHY, 0.05, 1.0), kd=(0, 1.0, 1.0), reject=True),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_doppler_accumulate_parity(n, dtype):
    """29 sums against the oracle at a lone pair, both sides of a wave, past
    one 256-thread workgroup, and several partial rows with a ragged tail; four
    kernel / rejection settings each; bit-identical on a second call. The
    bound is the project's for these float64-tree sums
    (test_colored_accumulate_parity)."""
    _lib, _ = _gpu()
    arrays, nt, prep = _accumulate_case(n, dtype)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    corr = arrays[5]
    threshold = 0.3   # one sigma of the dopplers' noise: rejects about a third
    for name, s in SETTINGS.items():
        want = dop.accumulate(*arrays, *prep, 0.1, s["reject"], threshold,
                              s["kg"], s["kd"], 0.01)
        got = []
        for _ in range(2):
            sums = torch.full((29,), -7.0, dtype=torch.float64, device="cuda")
            _lib.check(_accumulate(_lib, dev, n, nt, prep, 0.1, s["reject"],
                                   threshold, s["kg"], s["kd"], 0.01, sums),
                       "doppler_accumulate")
            torch.cuda.synchronize()
            got.append(sums.cpu().numpy())
        print(name, n, np.dtype(dtype).name, "max |diff|",
              np.abs(got[0] - want).max())
        assert got[0][28] == want[28] == (corr >= 0).sum(), name
        assert np.allclose(got[0], want, rtol=1e-11, atol=1e-9), name
        assert got[0].tobytes() == got[1].tobytes(), name
        if s["reject"] and n >= 63:
            _, rej = dop.pair_terms(*arrays, *prep, 0.1, True, threshold,
                                    s["kg"], s["kd"], 0.01)
            assert 0 < rej.sum() < rej.size


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_doppler_accumulate_without_pairs(dtype):
    """Every row -1, and n = 0: 29 zeros, status OK."""
    _lib, _ = _gpu()
    arrays, nt, prep = _accumulate_case(300, dtype)
    arrays[5][:] = -1
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    for n in (300, 0):
        sums = torch.full((29,), -7.0, dtype=torch.float64, device="cuda")
        st = _accumulate(_lib, dev, n, nt, prep, 0.1, False, 2.0, (0, 1, 1),
                         (0, 1, 1), 0.01, sums)
        torch.cuda.synchronize()
        assert st == 0, n
        assert np.array_equal(sums.cpu().numpy(), np.zeros(29)), n


@pytest.mark.parametrize("bad_index", ["nt", "below"])
def test_doppler_accumulate_rejects_an_index_outside_the_target(bad_index):
    """An index equal to nt (or below -1): INVALID_ARG, and the sums buffer
    keeps its previous contents."""
    _lib, _ = _gpu()
    arrays, nt, prep = _accumulate_case(700, np.float32)
    arrays[5][611] = nt if bad_index == "nt" else -2
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    sums = torch.full((29,), -7.0, dtype=torch.float64, device="cuda")
    st = _accumulate(_lib, dev, 700, nt, prep, 0.1, False, 2.0, (0, 1, 1),
                     (0, 1, 1), 0.01, sums)
    torch.cuda.synchronize()
    assert st == INVALID_ARG
    assert b"out of range" in _lib.lib().o3dmi_last_error()
    assert np.array_equal(sums.cpu().numpy(), np.full(29, -7.0))


def test_doppler_accumulate_argument_errors():
    _lib, _ = _gpu()
    arrays, nt, prep = _accumulate_case(64, np.float32)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    sums = torch.zeros(29, dtype=torch.float64, device="cuda")
    l2, l1 = (0, 1.0, 1.0), (dop.L1, 1.0, 1.0)
    assert _accumulate(_lib, dev, 64, nt, prep, 0.0, False, 2.0, l2, l2, 0.01,
                       sums) == INVALID_ARG
    assert _accumulate(_lib, dev, 64, nt, prep, 0.1, True, 2.0, l1, l2, 0.01,
                       sums) == UNSUPPORTED
    assert _accumulate(_lib, dev, 64, nt, prep, 0.1, True, 2.0, l2, l1, 0.01,
                       sums) == UNSUPPORTED
    # L1 without rejection is the reference's, and fine
    assert _accumulate(_lib, dev, 64, nt, prep, 0.1, False, 2.0, l1, l1, 0.01,
                       sums) == 0
    torch.cuda.synchronize()


def test_transformation_to_pose_through_the_library():
    _lib, reg = _gpu()
    rng = np.random.default_rng(3)
    for _ in range(20):
        T = orc.pose_to_transformation(
            np.concatenate([rng.uniform(-3, 3, 1), rng.uniform(-1.5, 1.5, 1),
                            rng.uniform(-3, 3, 4)]))
        assert np.array_equal(reg.transformation_to_pose(T),
                              dop.transformation_to_pose(T))
    T = np.eye(4)
    T[:3, :3] = [[0, np.sin(.3), np.cos(.3)], [0, np.cos(.3), -np.sin(.3)],
                 [-1, 0, 0]]
    assert np.array_equal(reg.transformation_to_pose(T),
                          dop.transformation_to_pose(T))


# ---- the driver ----------------------------------------------------------
_PAIRS = {}


def _doppler_pair(dtype, V=None, n=20000):
    """The synthetic room pair with directions (p / |p|) and dopplers of the
    true motion plus 2 cm/s of noise. Shared, read-only."""
    key = (np.dtype(dtype).name, None if V is None else V.tobytes(), n)
    if key not in _PAIRS:
        from open3d_amd import registration as reg
        from open3d_amd import synthetic as syn
        p = syn.make_icp_pair(n, n, seed=9, dtype=dtype)
        dirs = reg.compute_direction_vectors(p["source"])
        rng = np.random.default_rng(1)
        dops = dop.doppler_at(dirs, p["T_gt"],
                              dict(transform_vehicle_to_sensor=V))
        p["directions"] = np.ascontiguousarray(dirs)
        p["dopplers"] = np.ascontiguousarray(
            dops + (0.02 * rng.standard_normal(n)).astype(dtype))
        _PAIRS[key] = p
    return _PAIRS[key]


def _est(reg, params):
    kw = dict(params)
    for k in ("geometric_kernel", "doppler_kernel"):
        if k in kw:
            kw[k] = reg.RobustKernel(*kw[k])
    return reg.TransformationEstimationForDopplerICP(**kw)


def _run_both(reg, p, voxels, crits, dists, params, **kw):
    want = dop.multiscale_icp(p["source"], p["dopplers"], p["directions"],
                              p["target"], p["target_normals"], voxels, crits,
                              dists, params=params)
    got = reg.multi_scale_icp(
        torch.from_numpy(p["source"]).cuda(),
        torch.from_numpy(p["target"]).cuda(),
        torch.from_numpy(p["target_normals"]).cuda(), voxels,
        [reg.ICPConvergenceCriteria(*c) for c in crits], dists,
        estimation_method=_est(reg, params),
        source_dopplers=torch.from_numpy(p["dopplers"]).cuda(),
        source_directions=torch.from_numpy(p["directions"]).cuda(), **kw)
    return got, want


def _assert_same(got, want):
    ang, tr = _pose_err(got.transformation, want["transformation"])
    print("pose difference %.3g rad %.3g m; %d iterations, fitness %.6f"
          % (ang, tr, got.num_iterations, got.fitness))
    assert got.num_iterations == want["num_iterations"]
    assert got.converged == want["converged"]
    assert ang <= 1e-6 and tr <= 1e-5, (ang, tr)
    assert abs(got.fitness - want["fitness"]) < 1e-12


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["defaults", "switching",
                                  "switching_quarter_turn"])
def test_icp_doppler_pose_parity(dtype, case):
    """Single-scale ICP against the oracle driver: with every default; with
    the default switch-over iterations (2) made visible -- rejection of the
    pairs beyond 1.5 sigma of the dopplers' noise and a Tukey Doppler kernel
    that bites at 2 sigma, both from iteration 2; and the same with a
    vehicle-to-sensor transform whose rotation is an exact 90 degree turn
    about z (its float64 inverse is exact whatever computes it)."""
    _lib, reg = _gpu()
    V = V_LEVER if case.endswith("quarter_turn") else None
    p = _doppler_pair(dtype, V)
    params = {} if case == "defaults" else dict(
        reject_dynamic_outliers=True, doppler_outlier_threshold=0.03,
        doppler_kernel=(dop.TUKEY, 0.004, 1.0), transform_vehicle_to_sensor=V)
    got, want = _run_both(reg, p, [-1.0], [(1e-6, 1e-6, 30)], [0.07], params)
    assert want["num_iterations"] > 3
    _assert_same(got, want)
    ang, tr = _pose_err(got.transformation, p["T_gt"])
    assert ang < 2e-3 and tr < 5e-3, (ang, tr)


def test_icp_doppler_general_vehicle_rotation():
    """A general rotation in transform_vehicle_to_sensor: the inverse of the
    float64 rotation is taken (not the transpose of a cast matrix: the
    rotation here is scaled by 1.25, whose inverse is not its transpose)."""
    _lib, reg = _gpu()
    V = orc.pose_to_transformation([0.3, -0.2, 0.5, 0.4, -0.2, 0.3])
    V[:3, :3] *= 1.25
    p = _doppler_pair(np.float32, V)
    params = dict(transform_vehicle_to_sensor=V)
    got, want = _run_both(reg, p, [-1.0], [(1e-6, 1e-6, 30)], [0.07], params)
    _assert_same(got, want)
    wrong = dict(params)
    Vt = V.copy()
    Vt[:3, :3] = np.linalg.inv(V[:3, :3]).T
    wrong["transform_vehicle_to_sensor"] = Vt
    other = dop.multiscale_icp(p["source"], p["dopplers"], p["directions"],
                               p["target"], p["target_normals"], [-1.0],
                               [(1e-6, 1e-6, 30)], [0.07], params=wrong)
    ang, tr = _pose_err(other["transformation"], want["transformation"])
    assert tr > 1e-4, "the case does not tell an inverse from a transpose"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_multiscale_icp_doppler_three_scales(dtype):
    """Three scales with positive voxel sizes: the level sizes (read off the
    final correspondence set and the oracle's pyramid) and the pose match the
    oracle driver. Covers the 1-column attribute through the pyramid, the
    un-rotated directions, and the iteration index restarting per scale: the
    Doppler kernel switches on at iteration 2 of scale 0 and again at
    iteration 2 of scale 1 (each runs at least 3 iterations)."""
    _lib, reg = _gpu()
    p = _doppler_pair(dtype, V_LEVER)
    params = dict(doppler_robust_loss_min_iteration=2,
                  doppler_kernel=(dop.HUBER, 0.05, 1.0),
                  geometric_kernel=(dop.CAUCHY, 0.05, 1.0),
                  geometric_robust_loss_min_iteration=1,
                  transform_vehicle_to_sensor=V_LEVER)
    voxels, dists = [0.2, 0.1, 0.05], [0.4, 0.2, 0.1]
    crits = [(0, 0, 4), (0, 0, 4), (1e-6, 1e-6, 10)]
    log = []
    got, want = _run_both(reg, p, voxels, crits, dists, params,
                          callback_after_iteration=log.append)
    used = want["kernels_used"]
    assert len(used[0]) == 4 and len(used[1]) == 4
    l2 = (dop.L2, 1.0, 1.0)
    for k in (0, 1):
        assert [u[1] for u in used[k]] == [l2, l2, params["doppler_kernel"],
                                           params["doppler_kernel"]]
    assert [(c["scale_index"], c["scale_iteration_index"])
            for c in log[:8]] == [(s, i) for s in (0, 1) for i in range(4)]
    assert got.correspondence_set.shape[0] == want["level_sizes"][2][0]
    sizes = [want["level_sizes"][k][0] for k in range(3)]
    assert sizes[0] < sizes[1] < sizes[2] < p["source"].shape[0]
    # per-level sizes through the library's own VoxelDownSample
    pos = torch.from_numpy(p["source"]).cuda()
    for k in (2, 1, 0):
        pos, _ = reg.voxel_down_sample(pos, None, voxels[k])
        assert pos.shape[0] == sizes[k], k
    _assert_same(got, want)


def test_icp_doppler_on_the_degenerate_plane():
    """The scene of test_doppler_cpu (e) on the GPU: the pose equals the
    oracle's, i.e. the in-plane motion is recovered."""
    _lib, reg = _gpu()
    s = dop.plane_scene()
    got, want = _run_both(reg, s, [-1.0], [s["criteria"]], [s["max_dist"]], {})
    _assert_same(got, want)
    assert dop.in_plane_error(got.transformation, s["T_gt"]) < 1e-3


def test_compute_rmse_doppler_is_point_to_plane():
    _lib, reg = _gpu()
    dev = [torch.from_numpy(a.astype(np.float32)).cuda()
           for a in (SRC, TGT, TGT_N)] + [torch.from_numpy(CORR).cuda()]
    a = reg.compute_rmse(reg.TransformationEstimationForDopplerICP(), dev[0],
                         dev[1], dev[2], dev[3])
    b = reg.compute_rmse(reg.TransformationEstimationPointToPlane(), dev[0],
                         dev[1], dev[2], dev[3])
    assert a == b and abs(a - 0.335499) < 1e-5


def test_icp_doppler_argument_errors():
    _lib, reg = _gpu()
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    p = _doppler_pair(np.float32, None, n=2000)
    src, tgt, tn, dops, dirs = (torch.from_numpy(p[k]).cuda() for k in
                                ("source", "target", "target_normals",
                                 "dopplers", "directions"))
    est = reg.TransformationEstimationForDopplerICP
    with pytest.raises(ValueError, match="requires source pointcloud to have "
                                         "Doppler velocities"):
        reg.icp(src, tgt, tn, 0.07, estimation_method=est(),
                source_directions=dirs)
    with pytest.raises(ValueError, match="pre-computed direction vectors"):
        reg.icp(src, tgt, tn, 0.07, estimation_method=est(),
                source_dopplers=dops)
    with pytest.raises(ValueError, match="target pointcloud to have normals"):
        reg.icp(src, tgt, None, 0.07, estimation_method=est(),
                source_dopplers=dops, source_directions=dirs)

    def status(e):
        try:
            reg.icp(src, tgt, tn, 0.07, estimation_method=e,
                    source_dopplers=dops, source_directions=dirs)
        except RuntimeError as ex:
            return str(ex)
        return "ok"
    assert "period must be positive" in status(est(period=0.0))
    bad = np.eye(4)
    bad[1, 3] = np.inf
    assert "not finite" in status(est(transform_vehicle_to_sensor=bad))
    for k in ("geometric_kernel", "doppler_kernel"):
        kw = {k: reg.RobustKernel(reg.RobustKernel.L1Loss)}
        assert "L1Loss" in status(est(reject_dynamic_outliers=True, **kw))
        # L1Loss without rejection is the reference's and runs. One iteration,
        # both kernels on from iteration 0: the clouds are still centimetres
        # apart, so no residual is exactly 0. (Later iterations of this
        # noise-free room with axis-aligned normals reach p2plane residuals of
        # exactly 0 in Float32, where the reference's 1 / |r| weight times a
        # zero Jacobian entry is NaN: the solve then reports SINGULAR.)
        params = {k: (dop.L1, 1.0, 1.0), "doppler_robust_loss_min_iteration": 0}
        got, want = _run_both(reg, p, [-1.0], [(1e-6, 1e-6, 1)], [0.07],
                              params)
        assert np.isfinite(want["transformation"]).all()
        _assert_same(got, want)
    # the _ex entry has nowhere to take the parameters from
    crit = (_lib.IcpCriteria * 1)(_lib.IcpCriteria(1e-6, 1e-6, 3))
    one = np.array([-1.0]), np.array([0.07])
    res = _lib.RegistrationResultC()
    st = _lib.lib().o3dmi_registration_multiscale_icp_ex(
        _lib.ptr(src), src.shape[0], _lib.ptr(tgt), _lib.ptr(tn), tgt.shape[0],
        TORCH_TO_O3DMI[src.dtype], 1, _lib.f64p(one[0]), crit,
        _lib.f64p(one[1]), None, 4, None, None, 0, C.c_double(1.0),
        C.c_double(1.0), _lib.ICP_CALLBACK(0), None, _lib.ALLREDUCE_SUM(0),
        None, None, C.byref(res), stream())
    assert st == INVALID_ARG
    # and the statuses behind the messages
    d = _lib.IcpDoppler()
    est(period=0.0)._fill(d)
    d.source_dopplers, d.source_directions = dops.data_ptr(), dirs.data_ptr()

    def call(d):
        return _lib.lib().o3dmi_registration_multiscale_icp_doppler(
            _lib.ptr(src), src.shape[0], _lib.ptr(tgt), _lib.ptr(tn),
            tgt.shape[0], TORCH_TO_O3DMI[src.dtype], 1, _lib.f64p(one[0]),
            crit, _lib.f64p(one[1]), None, C.byref(d), None,
            _lib.ICP_CALLBACK(0), None, _lib.ALLREDUCE_SUM(0), None, None,
            C.byref(res), stream())
    assert call(d) == INVALID_ARG
    est(reject_dynamic_outliers=True,
        doppler_kernel=reg.RobustKernel(reg.RobustKernel.L1Loss))._fill(d)
    assert call(d) == UNSUPPORTED
    est()._fill(d)
    d.source_dopplers = None
    assert call(d) == INVALID_ARG
    torch.cuda.synchronize()


def test_multiscale_icp_doppler_level_sharded_two_ranks_equal_one_rank():
    """level_sharding with a communicator of two ranks (two host threads over
    the in-process transport of test_configs_gpu): the driver slices dopplers
    and directions with the positions of every level, so both ranks end with
    the unsharded run's iteration count and pose (to the rounding of the
    float64 sums), and their correspondence rows tile the unsharded set."""
    _lib, reg = _gpu()
    from open3d_amd.sharding import Comm
    from test_configs_gpu import _Loopback, _run_ranks
    p = _doppler_pair(np.float32, V_LEVER)
    dev = {k: torch.from_numpy(p[k]).cuda() for k in
           ("source", "target", "target_normals", "dopplers", "directions")}
    voxels, dists = [0.1, 0.05], [0.2, 0.1]
    crit = [reg.ICPConvergenceCriteria(1e-6, 1e-6, n) for n in (6, 10)]
    est = reg.TransformationEstimationForDopplerICP(
        transform_vehicle_to_sensor=V_LEVER,
        doppler_kernel=reg.RobustKernel(dop.HUBER, 0.05))

    def run(**kw):
        return reg.multi_scale_icp(
            dev["source"].clone(), dev["target"], dev["target_normals"],
            voxels, crit, dists, estimation_method=est,
            source_dopplers=dev["dopplers"],
            source_directions=dev["directions"], **kw)
    one = run()
    torch.cuda.synchronize()
    world = 2
    lb = _Loopback(world)

    def rank_body(r):
        comm = lb.comm(r)
        comm.install()
        try:
            out = run(level_sharding=True)
            torch.cuda.synchronize()
        finally:
            Comm.uninstall()
        lb.bar.wait()
        comm.destroy()
        return out
    got = _run_ranks(world, rank_body)
    n_rows = one.correspondence_set.shape[0]
    union = torch.full((n_rows,), -1, dtype=torch.int64, device="cuda")
    for r in range(world):
        assert got[r].num_iterations == one.num_iterations, r
        d = np.abs(got[r].transformation - one.transformation).max()
        assert d <= 1e-9, (r, d)
        assert abs(got[r].fitness - one.fitness) < 1e-12
        c = got[r].correspondence_set
        assert c.shape[0] == n_rows
        mine = c >= 0
        assert not bool((union[mine] >= 0).any())
        union[mine] = c[mine]
    assert np.array_equal(got[0].transformation, got[1].transformation)
    assert torch.equal(union, one.correspondence_set)
