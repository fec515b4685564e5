"""Generalized ICP (TransformationEstimationForGeneralizedICP) on the GPU
against the numpy oracle of _gicp_oracle.py: the covariances from normals, the
accumulate kernel, the covariance columns through the pyramid, the driver."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gicp_oracle as gicp
import _oracle as orc
from test_gicp_cpu import K, MEASURED_ROUTE_RATIO

pytestmark = pytest.mark.gpu

INVALID_ARG = 1


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
    return None if a is None else np.ascontiguousarray(
        a, np.float64).ctypes.data_as(C.POINTER(C.c_double))


# ---- covariances from normals ------------------------------------------------
BRANCH_NORMALS = [[-0.995, 0.0999, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0],
                  [0.0, 2.0, 0.0]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_covariances_from_normals_bit_equal(n, dtype):
    """Noisy unit normals with the branch cases planted (the cap c < -0.99,
    e1, -e1, a non-unit normal): the oracle's bits."""
    _lib, reg = _gpu()
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    m = min(n, len(BRANCH_NORMALS))
    x[:m] = BRANCH_NORMALS[:m]
    x = np.ascontiguousarray(x.astype(dtype))
    want = gicp.covariances_from_normals(x, 1e-3)
    got = reg.covariances_from_normals(torch.from_numpy(x).cuda(), 1e-3)
    got = got.cpu().numpy()
    print(n, np.dtype(dtype).name, "values that differ:",
          int((got != want).sum()))
    assert got.shape == (n, 3, 3) and got.dtype == dtype
    assert got.tobytes() == want.tobytes()


def test_covariances_from_normals_rejects_epsilon_zero():
    _lib, reg = _gpu()
    from open3d_amd.core import stream
    x = torch.ones((8, 3), dtype=torch.float32, device="cuda")
    out = torch.full((8, 3, 3), -7.0, dtype=torch.float32, device="cuda")
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        st = _lib.lib().o3dmi_pointcloud_covariances_from_normals(
            _lib.ptr(x), 8, _lib.F32, C.c_double(eps), _lib.ptr(out), stream())
        assert st == INVALID_ARG, eps
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- the accumulate seam -----------------------------------------------------
def _accumulate(_lib, dev, n, nt, R, kernel, sums):
    """o3dmi_icp_generalized_accumulate on device tensors dev = (src, src_cov,
    tgt, tgt_cov, corr) -> status."""
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    dt = next(t for t in dev if t is not None).dtype
    return _lib.lib().o3dmi_icp_generalized_accumulate(
        *[_lib.ptr(t) for t in dev], n, nt,
        TORCH_TO_O3DMI.get(dt, _lib.F32), _f64p(R), kernel[0],
        C.c_double(kernel[1]), C.c_double(kernel[2]), _lib.ptr(sums), stream())


def _assert_within_bound(got, want, abs_sums, what):
    """|got - want| <= K 2^-52 sum |term| per entry of [0..28]."""
    bound = K * 2.0 ** -52 * abs_sums
    diff = np.abs(got[:29] - want[:29])
    with np.errstate(all="ignore"):
        used = np.where(bound > 0, diff / bound, 0.0).max()
    print(what, "largest |diff| / bound %.3g (K = %g, measured route ratio %g)"
          % (used, K, MEASURED_ROUTE_RATIO))
    assert np.all(diff <= bound), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", gicp.SIZES)
def test_generalized_accumulate_parity(n, dtype):
    """32 sums against the oracle at a lone pair, both sides of a wave, past
    one 256-thread workgroup, and several partial rows with a ragged tail; four
    robust kernels each under a non-identity R_source9; bit-identical on a
    second call."""
    _lib, _ = _gpu()
    arrays, nt = gicp.accumulate_case(n, dtype)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    corr = arrays[4]
    R = gicp.r_source()
    for name, kernel in gicp.SETTINGS.items():
        want, abs_sums = gicp.accumulate(*arrays, R, kernel)
        got = []
        for _ in range(2):
            sums = torch.full((32,), -7.0, dtype=torch.float64, device="cuda")
            _lib.check(_accumulate(_lib, dev, n, nt, R, kernel, sums),
                       "generalized_accumulate")
            torch.cuda.synchronize()
            got.append(sums.cpu().numpy())
        assert got[0][28] == want[28] == (corr >= 0).sum(), name
        assert got[0][29] == 0 and got[0][30] == 0 and got[0][31] == 0, name
        _assert_within_bound(got[0], want, abs_sums,
                             "%s n=%d %s" % (name, n, np.dtype(dtype).name))
        assert got[0].tobytes() == got[1].tobytes(), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_generalized_accumulate_counts_pairs_that_cannot_be_whitened(dtype):
    """Cs = Ct = diag(1,1,0) under R = I on four rows and a NaN covariance on
    one: [29] counts them, [0..28] are the oracle's, which skips them."""
    _lib, _ = _gpu()
    arrays, nt = gicp.accumulate_case(300, dtype)
    src, cs, tgt, ct, corr = arrays
    rows = np.nonzero(corr >= 0)[0][[3, 50, 120, 200, 77]]
    flat = np.diag([1.0, 1.0, 0.0]).astype(dtype)
    cs[rows[:4]] = flat
    ct[corr[rows[:4]]] = flat
    cs[rows[4], 1, 1] = np.nan
    want, abs_sums = gicp.accumulate(*arrays, None, (gicp.L2, 1.0, 1.0))
    assert want[29] == 5
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    sums = torch.full((32,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_accumulate(_lib, dev, 300, nt, None, (0, 1.0, 1.0), sums),
               "generalized_accumulate")
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    assert got[29] == 5 and got[28] == want[28] == (corr >= 0).sum() - 5
    assert got[30] == 0 and got[31] == 0
    _assert_within_bound(got, want, abs_sums, np.dtype(dtype).name)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_generalized_accumulate_without_pairs(dtype):
    """Every row -1, and n = 0: 32 zeros, status OK."""
    _lib, _ = _gpu()
    arrays, nt = gicp.accumulate_case(300, dtype)
    arrays[4][:] = -1
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    for n in (300, 0):
        sums = torch.full((32,), -7.0, dtype=torch.float64, device="cuda")
        st = _accumulate(_lib, dev, n, nt, None, (0, 1.0, 1.0), sums)
        torch.cuda.synchronize()
        assert st == 0, n
        assert np.array_equal(sums.cpu().numpy(), np.zeros(32)), n


@pytest.mark.parametrize("bad_index", ["nt", "below"])
def test_generalized_accumulate_rejects_an_index_outside_the_target(bad_index):
    """An index equal to nt (or -2): INVALID_ARG, and the sums buffer keeps
    its previous contents."""
    _lib, _ = _gpu()
    arrays, nt = gicp.accumulate_case(700, np.float32)
    arrays[4][611] = nt if bad_index == "nt" else -2
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    sums = torch.full((32,), -7.0, dtype=torch.float64, device="cuda")
    st = _accumulate(_lib, dev, 700, nt, None, (0, 1.0, 1.0), sums)
    torch.cuda.synchronize()
    assert st == INVALID_ARG
    assert b"out of range" in _lib.lib().o3dmi_last_error()
    assert np.array_equal(sums.cpu().numpy(), np.full(32, -7.0))


# ---- the driver --------------------------------------------------------------
_PAIRS = {}
ICP_ARGS = ([-1.0], [(1e-6, 1e-6, 30)], [0.07])


def _pair(dtype, n=20000):
    """The synthetic room pair with both clouds' normals from the oracle's
    EstimateNormals(KNN 20) and the covariances from those. Shared,
    read-only."""
    key = (np.dtype(dtype).name, n)
    if key not in _PAIRS:
        from open3d_amd import synthetic as syn
        p = syn.make_icp_pair(n, n, seed=9, dtype=dtype)
        for side in ("source", "target"):
            nrm = gicp.estimate_normals_knn(p[side], 20)
            p[side + "_normals_knn"] = nrm
            p[side + "_covariances"] = gicp.covariances_from_normals(nrm, 1e-3)
        _PAIRS[key] = p
    return _PAIRS[key]


def _cuda(a):
    return None if a is None else torch.from_numpy(
        np.ascontiguousarray(a)).cuda()


def _run_both(reg, source, target, voxels, crits, dists, init=None,
              kernel=(gicp.L2, 1.0, 1.0), source_covariances=None,
              target_covariances=None, source_normals=None,
              target_normals=None, **kw):
    want = gicp.multiscale_icp(
        source, target, voxels, crits, dists, init=init, kernel=kernel,
        source_covariances=source_covariances,
        target_covariances=target_covariances, source_normals=source_normals,
        target_normals=target_normals)
    est = reg.TransformationEstimationForGeneralizedICP(
        1e-3, reg.RobustKernel(*kernel))
    got, singular = reg.multi_scale_icp(
        _cuda(source), _cuda(target), _cuda(target_normals), voxels,
        [reg.ICPConvergenceCriteria(*c) for c in crits], dists,
        init_source_to_target=init, estimation_method=est,
        source_normals=_cuda(source_normals),
        source_covariances=_cuda(source_covariances),
        target_covariances=_cuda(target_covariances),
        return_singular_pairs=True, **kw)
    assert singular == want["singular_pairs"]
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
@pytest.mark.parametrize("case", ["given", "from_normals", "estimated",
                                  "given_tukey"])
def test_icp_generalized_pose_parity(dtype, case):
    """Single-scale ICP against the oracle driver with the covariances given,
    made from given normals, and made from normals the driver estimates; and
    once with a Tukey kernel that zeroes the first iterations' residuals along
    the normals (whitened, 5 cm are about 1.1; the kernel ends at 0.5)."""
    _lib, reg = _gpu()
    p = _pair(dtype)
    kw = {}
    if case.startswith("given"):
        kw = dict(source_covariances=p["source_covariances"],
                  target_covariances=p["target_covariances"])
    elif case == "from_normals":
        kw = dict(source_normals=p["source_normals_knn"],
                  target_normals=p["target_normals_knn"])
    if case == "given_tukey":
        kw["kernel"] = (gicp.TUKEY, 0.5, 1.0)
    got, want = _run_both(reg, p["source"], p["target"], *ICP_ARGS, **kw)
    assert want["num_iterations"] > 3
    _assert_same(got, want)
    ang, tr = _pose_err(got.transformation, p["T_gt"])
    assert ang < 2e-3 and tr < 5e-3, (ang, tr)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_multiscale_icp_generalized_three_scales(dtype):
    """Three scales with positive voxel sizes: the level sizes (read off the
    final correspondence set and the library's own VoxelDownSample against
    the oracle's pyramid) and the pose match the oracle driver -- the
    covariance columns through the pyramid."""
    _lib, reg = _gpu()
    p = _pair(dtype)
    voxels, dists = [0.2, 0.1, 0.05], [0.4, 0.2, 0.1]
    crits = [(0, 0, 4), (0, 0, 4), (1e-6, 1e-6, 10)]
    got, want = _run_both(reg, p["source"], p["target"], voxels, crits, dists,
                          source_covariances=p["source_covariances"],
                          target_covariances=p["target_covariances"])
    sizes = [want["level_sizes"][k][0] for k in range(3)]
    assert sizes[0] < sizes[1] < sizes[2] < p["source"].shape[0]
    assert got.correspondence_set.shape[0] == sizes[2]
    pos = torch.from_numpy(p["source"]).cuda()
    for k in (2, 1, 0):
        pos, _ = reg.voxel_down_sample(pos, None, voxels[k])
        assert pos.shape[0] == sizes[k], k
    assert want["num_iterations"] > 8
    _assert_same(got, want)
    ang, tr = _pose_err(got.transformation, p["T_gt"])
    assert ang < 2e-3 and tr < 5e-3, (ang, tr)


def test_icp_generalized_rotates_the_source_covariances():
    """The source turned away by half a radian, its covariances given in its
    own frame, the turn given back as the init: the driver rotates the
    covariances with the cumulative transformation. An oracle run that leaves
    them unrotated ends more than 1e-4 rad away."""
    _lib, reg = _gpu()
    p = _pair(np.float64)
    Q = orc.pose_to_transformation([0.3, -0.25, 0.3, 0.1, -0.2, 0.05])
    Qi = np.linalg.inv(Q)
    source = np.ascontiguousarray(p["source"] @ Qi[:3, :3].T + Qi[:3, 3])
    cs = gicp.covariances_from_normals(gicp.estimate_normals_knn(source, 20))
    got, want = _run_both(reg, source, p["target"], *ICP_ARGS, init=Q,
                          source_covariances=cs,
                          target_covariances=p["target_covariances"])
    _assert_same(got, want)
    ang, tr = _pose_err(got.transformation, p["T_gt"] @ Q)
    assert ang < 2e-3 and tr < 5e-3, (ang, tr)
    unrotated = gicp.multiscale_icp(
        source, p["target"], *ICP_ARGS, init=Q, source_covariances=cs,
        target_covariances=p["target_covariances"], rotate_covariances=False)
    ang, _ = _pose_err(unrotated["transformation"], got.transformation)
    assert ang > 1e-4, "the case does not tell a rotated covariance"


def test_icp_generalized_argument_errors():
    _lib, reg = _gpu()
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    arrays, nt = gicp.accumulate_case(64, np.float32)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    sums = torch.full((32,), -7.0, dtype=torch.float64, device="cuda")
    l2 = (0, 1.0, 1.0)
    # NULL tables, a kernel id of 7
    for hole in (1, 3):
        holed = list(dev)
        holed[hole] = None
        assert _accumulate(_lib, holed, 64, nt, None, l2, sums) == INVALID_ARG
    assert _accumulate(_lib, dev, 64, nt, None, (7, 1.0, 1.0),
                       sums) == INVALID_ARG
    assert _accumulate(_lib, dev, 64, nt, None, l2, sums) == 0
    torch.cuda.synchronize()
    # the _ex entry has nowhere to take the estimator's parameters from
    src, tgt = dev[0], dev[2]
    crit = (_lib.IcpCriteria * 1)(_lib.IcpCriteria(1e-6, 1e-6, 3))
    one = np.array([-1.0]), np.array([0.07])
    res = _lib.RegistrationResultC()
    st = _lib.lib().o3dmi_registration_multiscale_icp_ex(
        _lib.ptr(src), 64, _lib.ptr(tgt), None, nt, TORCH_TO_O3DMI[src.dtype],
        1, _lib.f64p(one[0]), crit, _lib.f64p(one[1]), None, 5, None, None, 0,
        C.c_double(1.0), C.c_double(1.0), _lib.ICP_CALLBACK(0), None,
        _lib.ALLREDUCE_SUM(0), None, None, C.byref(res), stream())
    assert st == INVALID_ARG

    def call(g, ns=64):
        return _lib.lib().o3dmi_registration_multiscale_icp_generalized(
            _lib.ptr(src), ns, _lib.ptr(tgt), None, nt,
            TORCH_TO_O3DMI[src.dtype], 1, _lib.f64p(one[0]), crit,
            _lib.f64p(one[1]), None, C.byref(g) if g is not None else None,
            None, _lib.ICP_CALLBACK(0), None, _lib.ALLREDUCE_SUM(0), None,
            None, C.byref(res), stream())
    g = _lib.IcpGeneralized()
    g.source_covariances = dev[1].data_ptr()
    g.target_covariances = dev[3].data_ptr()
    g.epsilon = 0.0
    assert call(g) == INVALID_ARG
    g.epsilon = 1e-3
    g.robust_kernel = 7
    assert call(g) == INVALID_ARG
    assert call(None) == INVALID_ARG
    # neither covariances nor normals on a source of two points: whatever
    # EstimateNormals(KNN 20) answers for that cloud, unchanged
    nrm = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
    want_st = _lib.lib().o3dmi_pointcloud_estimate_normals(
        _lib.ptr(src), 2, TORCH_TO_O3DMI[src.dtype], 20, C.c_double(-1.0),
        _lib.ptr(nrm), 0, stream())
    want_msg = _lib.lib().o3dmi_last_error()
    assert want_st != 0
    g.robust_kernel = 0
    g.source_covariances = None
    assert call(g, ns=2) == want_st
    assert _lib.lib().o3dmi_last_error() == want_msg
    torch.cuda.synchronize()
    # the Python mirror's own checks
    est = reg.TransformationEstimationForGeneralizedICP()
    with pytest.raises(ValueError, match=r"must be \{N,3,3\}"):
        reg.icp(src, tgt, None, 0.07, estimation_method=est,
                source_covariances=dev[1][:10])
    with pytest.raises(ValueError, match="return_singular_pairs"):
        reg.icp(src, tgt, None, 0.07, return_singular_pairs=True,
                estimation_method=reg.TransformationEstimationPointToPoint())


def test_multiscale_icp_generalized_level_sharded_two_ranks_equal_one_rank():
    """level_sharding with a communicator of two ranks (two host threads over
    the in-process transport of test_configs_gpu): the driver slices the
    covariance tables with the positions of every level, so both ranks end
    with the unsharded run's iteration count and pose (to the rounding of the
    float64 sums), and their correspondence rows tile the unsharded set."""
    _lib, reg = _gpu()
    from open3d_amd.sharding import Comm
    from test_configs_gpu import _Loopback, _run_ranks
    p = _pair(np.float32)
    dev = {k: _cuda(p[k]) for k in ("source", "target", "source_covariances",
                                    "target_covariances")}
    voxels, dists = [0.1, 0.05], [0.2, 0.1]
    crit = [reg.ICPConvergenceCriteria(1e-6, 1e-6, n) for n in (6, 10)]
    est = reg.TransformationEstimationForGeneralizedICP(
        kernel=reg.RobustKernel(gicp.HUBER, 0.5))

    def run(**kw):
        return reg.multi_scale_icp(
            dev["source"].clone(), dev["target"], None, voxels, crit, dists,
            estimation_method=est,
            source_covariances=dev["source_covariances"],
            target_covariances=dev["target_covariances"], **kw)
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


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compute_rmse_generalized(dtype):
    """sqrt(sum d^T W d / count) against the oracle at n = 257; no
    correspondence: 0.0; a pair that cannot be whitened stays in the count."""
    _lib, reg = _gpu()
    arrays, nt = gicp.accumulate_case(257, dtype)
    est = reg.TransformationEstimationForGeneralizedICP()

    def rmse(arrays):
        src, cs, tgt, ct, corr = (torch.from_numpy(a).cuda() for a in arrays)
        return reg.compute_rmse(est, src, tgt, None, corr,
                                source_covariances=cs, target_covariances=ct)
    want = gicp.compute_rmse(*arrays)
    got = rmse(arrays)
    print(np.dtype(dtype).name, "rmse", got, "relative difference",
          abs(got - want) / want)
    assert abs(got - want) <= 1e-12 * want
    row = int(np.nonzero(arrays[4] >= 0)[0][5])
    planted = [a.copy() for a in arrays]
    planted[1][row] = np.nan
    want = gicp.compute_rmse(*planted)
    assert abs(rmse(planted) - want) <= 1e-12 * want
    none = [a.copy() for a in arrays]
    none[4][:] = -1
    assert rmse(none) == 0.0
