"""MultiScaleICP pyramids across the tiled VoxelDownSample's 2^20-point limit.

The source and the target pyramid are built in the same launches
(VdsPairAsync) while both clouds fit the tiled form (kTiledMaxPoints = 2^20
points); a pair that does not falls back to one call per cloud, the larger
ones on the sort form. Every case here compares HIP with the CPU oracle
(pose within 1e-6 rad / 1e-5 m, equal iteration counts and fitness) and, per
iteration, the callback logs: the same scale sequence, fitness within 1e-12
and rmse within 1e-6. Fitness is inliers over the level's size, so the logs
pin the size of every level of both pyramids, not just the final result.
Three or more down-sampled scales: with two, a wrongly zeroed level count
has no level left to show on."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import _oracle as orc
from test_icp_gpu import _color_field, _pose_err

pytestmark = pytest.mark.gpu

N = 1 << 20  # kTiledMaxPoints
BIG = 1_500_000
VS3 = [0.05, 0.025, 0.0125]
MD3 = [0.15, 0.075, 0.0375]
CRIT3 = [(1e-6, 1e-6, 20), (1e-6, 1e-6, 10), (1e-6, 1e-6, 5)]
VS4 = VS3 + [0.00625]
MD4 = MD3 + [0.01875]
CRIT4 = CRIT3 + [(1e-6, 1e-6, 3)]
KEY_RANGE = 4  # O3DMI_ERR_KEY_RANGE


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib, registration
    return _lib, registration


def _color_gradients(P, nrm):
    """The analytic gradient of _color_field's intensity (mean of the three
    channels) in the tangent plane: gradients a caller hands in."""
    P = P.astype(np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    a = 0.4 * np.cos(3 * x + 2 * y)
    b = -0.4 * np.sin(2 * y - z)
    c = 0.3 * np.cos(4 * z + x)
    g = np.stack([3 * a + c, 2 * a + 2 * b, -b + 4 * c], 1) / 3.0
    n = nrm.astype(np.float64)
    g -= np.sum(g * n, 1, keepdims=True) * n
    return g


@pytest.fixture(scope="module")
def clouds():
    """One large pair per dtype (same geometry: make_icp_pair draws in
    float64), made on first use; every case slices prefixes from it."""
    _gpu()
    orc.set_threads(min(16, os.cpu_count() or 1))
    made = {}

    def get(dtype):
        if dtype not in made:
            from open3d_amd import synthetic as syn
            made[dtype] = syn.make_icp_pair(BIG, BIG, seed=31, dtype=dtype)
        return made[dtype]
    return get


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _estimation(reg, kind):
    if kind == "point":
        return reg.TransformationEstimationPointToPoint()
    if kind == "symmetric":
        return reg.TransformationEstimationSymmetric(
            reg.RobustKernel(reg.RobustKernel.TukeyLoss, 0.1))
    if kind == "colored":
        return reg.TransformationEstimationForColoredICP(
            0.9, reg.RobustKernel(reg.RobustKernel.TukeyLoss, 0.1))
    return reg.TransformationEstimationPointToPlane()


def _problem(p, ns, nt, kind="plane", gradients=False):
    """Host arrays of one registration problem: prefixes of the pair plus
    what the estimator reads."""
    dt = p["source"].dtype
    q = dict(source=np.ascontiguousarray(p["source"][:ns]),
             target=np.ascontiguousarray(p["target"][:nt]),
             target_normals=np.ascontiguousarray(p["target_normals"][:nt]))
    if kind == "symmetric":
        # source normals as test_multiscale_icp_symmetric makes them (the
        # nearest target point's; a smaller radius at these densities)
        idx, _, _ = orc.hybrid_search(
            q["target"], orc.transform_points(p["T_gt"], q["source"]), 0.02,
            1)
        q["source_normals"] = np.ascontiguousarray(orc.transform_normals(
            np.linalg.inv(p["T_gt"]),
            q["target_normals"][np.maximum(idx[:, 0], 0)]).astype(dt))
    if kind == "colored":
        q["source_colors"] = np.ascontiguousarray(_color_field(
            orc.transform_points(p["T_gt"], q["source"])).astype(dt))
        q["target_colors"] = np.ascontiguousarray(
            _color_field(q["target"]).astype(dt))
        if gradients:
            q["target_color_gradients"] = np.ascontiguousarray(
                _color_gradients(q["target"], q["target_normals"]).astype(dt))
    return q


_ORACLE_KW = {"plane": dict(estimation=0),
              "point": dict(estimation=1),
              "symmetric": dict(estimation=2, kernel=(5, 0.1, 1.0)),
              "colored": dict(estimation=3, kernel=(5, 0.1, 1.0),
                              lambda_geometric=0.9)}


def _oracle(q, vs, crit, md, kind):
    log = []
    kw = dict(_ORACLE_KW[kind])
    for k in ("source_normals", "source_colors", "target_colors",
              "target_color_gradients"):
        if k in q:
            kw[k] = q[k]
    # gradients the driver estimates itself: the product's converged solve
    orc.set_exact_color_gradients(kind == "colored")
    try:
        want = orc.multiscale_icp(
            q["source"], q["target"],
            None if kind == "point" else q["target_normals"], vs, crit, md,
            accumulate_double=True, callback=log.append, **kw)
    finally:
        orc.set_exact_color_gradients(False)
    assert want["status"] == 0
    return want, log


def _hip(reg, q, vs, crit, md, kind):
    log = []
    kw = {}
    for k in ("source_normals", "source_colors", "target_colors",
              "target_color_gradients"):
        if k in q:
            kw[k] = _dev(q[k])
    got = reg.multi_scale_icp(
        _dev(q["source"]), _dev(q["target"]),
        None if kind == "point" else _dev(q["target_normals"]), vs,
        [reg.ICPConvergenceCriteria(*c) for c in crit], md,
        estimation_method=_estimation(reg, kind),
        callback_after_iteration=log.append, **kw)
    return got, log


def _check(got, glog, want, wlog, n_scales):
    ang, tr = _pose_err(want["transformation"], got.transformation)
    assert ang <= 1e-6 and tr <= 1e-5, (ang, tr)
    assert got.num_iterations == want["num_iterations"]
    assert abs(got.fitness - want["fitness"]) < 1e-12, (got.fitness,
                                                        want["fitness"])
    # every scale ran, in the oracle's order, on levels of the oracle's sizes
    assert [e["scale_index"] for e in glog] == \
        [e["scale_index"] for e in wlog]
    assert sorted(set(e["scale_index"] for e in glog)) == \
        list(range(n_scales))
    for g, w in zip(glog, wlog):
        assert abs(g["fitness"] - w["fitness"]) < 1e-12, (
            g["scale_index"], g["fitness"], w["fitness"])
        assert abs(g["inlier_rmse"] - w["inlier_rmse"]) < 1e-6, (
            g["scale_index"], g["inlier_rmse"], w["inlier_rmse"])
    assert all(e["fitness"] > 0.5 for e in glog)


def _parity(reg, p, ns, nt, vs, crit, md, kind="plane", gradients=False):
    q = _problem(p, ns, nt, kind, gradients)
    want, wlog = _oracle(q, vs, crit, md, kind)
    got, glog = _hip(reg, q, vs, crit, md, kind)
    _check(got, glog, want, wlog, len(vs))


# (ns, nt, dtype, voxel sizes): point-to-plane at every side of the limit
_ROWS = {
    "paired_tiled_at_limit": (N, N, np.float32, VS3),
    "mixed_source_tiled": (N, N + 1, np.float32, VS3),
    "mixed_target_tiled": (N + 1, N, np.float64, VS3),
    "mixed_4_scales": (900_000, 1_200_000, np.float64, VS4),
    "both_sort_form": (1_200_000, 1_100_000, np.float32, VS3),
}


@pytest.mark.parametrize("row", list(_ROWS))
def test_multiscale_icp_point_to_plane_across_the_tiled_limit(clouds, row):
    """2^20 / 2^20: the largest pair built in the same launches, whose
    coarsest reduce launch posts both chains' counts itself. One point more
    on either side: one cloud tiled, the other on the sort form, one call
    each (the counts then go out by the separate posting launch, and the
    tiled cloud's call must not post them first). Both beyond: two sorts."""
    _lib, reg = _gpu()
    ns, nt, dtype, vs = _ROWS[row]
    md = MD4 if len(vs) == 4 else MD3
    crit = CRIT4 if len(vs) == 4 else CRIT3
    _parity(reg, clouds(dtype), ns, nt, vs, crit, md)


@pytest.mark.parametrize("kind,ns,nt", [("point", N, N + 1),
                                        ("symmetric", N + 1, N)])
def test_multiscale_icp_other_estimators_on_a_mixed_pair(clouds, kind, ns,
                                                         nt):
    """Point-to-point (positions only) and symmetric (source normals averaged
    too) on a pair that straddles the limit."""
    _lib, reg = _gpu()
    _parity(reg, clouds(np.float32), ns, nt, VS3, CRIT3, MD3, kind)


@pytest.mark.parametrize("given_gradients", [True, False])
def test_multiscale_icp_colored_on_a_mixed_pair(clouds, given_gradients):
    """Coloured ICP builds its pyramids as two chains (three attribute passes
    per target level); the gradients are handed in (and averaged down the
    pyramid) or estimated on the finest level (which waits for its size)."""
    _lib, reg = _gpu()
    _parity(reg, clouds(np.float32), N, N + 1, VS3, CRIT3, MD3, "colored",
            gradients=given_gradients)


def test_multiscale_icp_finest_level_is_the_input_on_a_mixed_pair(clouds):
    """voxel_sizes [0.05, -1]: the coarsest level is the pair's only
    down-sampled one, its size read back through the chain's counts."""
    _lib, reg = _gpu()
    _parity(reg, clouds(np.float32), N + 1, N, [0.05, -1.0],
            [(1e-6, 1e-6, 20), (1e-6, 1e-6, 3)], [0.15, 0.05])


def test_multiscale_icp_device_counts_with_capacities_across_the_limit(
        clouds):
    """o3dmi_icp_options_t ns_dev / nt_dev: the buffers' capacities (2^20,
    2^20 + 4096) size the pyramid's launches -- a mixed pair -- while the
    live sizes (1 000 000, 1 040 000) would both fit the tiled form. The
    result is the same bits as the call given exact-size tensors, and
    matches the oracle."""
    _lib, reg = _gpu()
    p = clouds(np.float32)
    ns, nt, cap_s, cap_t = 1_000_000, 1_040_000, N, N + 4096
    q = _problem(p, ns, nt)
    want, wlog = _oracle(q, VS3, CRIT3, MD3, "plane")
    exact, elog = _hip(reg, q, VS3, CRIT3, MD3, "plane")
    _check(exact, elog, want, wlog, 3)
    # rows past the live sizes hold junk the call must never look at
    src_buf = _dev(p["source"][:cap_s])
    src_buf[ns:] = float("nan")
    tgt_buf = _dev(p["target"][:cap_t])
    nrm_buf = _dev(p["target_normals"][:cap_t])
    tgt_buf[nt:] = 1e6
    nrm_buf[nt:] = float("nan")
    counts = torch.tensor([ns, nt], dtype=torch.int32, device="cuda")
    log = []
    got = reg.multi_scale_icp(src_buf, tgt_buf, nrm_buf, VS3,
                              [reg.ICPConvergenceCriteria(*c) for c in CRIT3],
                              MD3, callback_after_iteration=log.append,
                              device_counts=(counts[0:1], counts[1:2]))
    assert np.array_equal(got.transformation, exact.transformation)
    assert got.num_iterations == exact.num_iterations
    assert got.fitness == exact.fitness
    assert got.inlier_rmse == exact.inlier_rmse
    assert [(e["scale_index"], e["fitness"], e["inlier_rmse"]) for e in log] \
        == [(e["scale_index"], e["fitness"], e["inlier_rmse"]) for e in elog]


_KEY_RANGE_CASES = {
    # (ns, nt, estimator, which cloud holds the far point)
    "mixed_small_cloud": (N, N + 1, "plane", "source"),
    "mixed_large_cloud": (N, N + 1, "plane", "target"),
    "tiled_pair": (60_000, 60_000, "plane", "target"),
    "colored_pair": (N, N + 1, "colored", "source"),
}


@pytest.mark.parametrize("case", list(_KEY_RANGE_CASES))
def test_multiscale_icp_raises_the_key_range_error(clouds, case):
    """A voxel coordinate outside +-2^20 is O3DMI_ERR_KEY_RANGE wherever the
    point sits: in the tiled or the sort-form cloud of a mixed pair, in a
    pair built in the same launches, in a coloured pair's chains. The chain
    abandoned by the error is cleaned up: a clean call after it gives the
    bits it gave before."""
    _lib, reg = _gpu()
    ns, nt, kind, where = _KEY_RANGE_CASES[case]
    q = _problem(clouds(np.float32), ns, nt, kind, gradients=True)
    crit = [(1e-6, 1e-6, 4)] * 3

    def run(problem):
        r, log = _hip(reg, problem, VS3, crit, MD3, kind)
        return (r.transformation.tobytes(), r.num_iterations, r.fitness,
                r.inlier_rmse, [(e["fitness"], e["inlier_rmse"]) for e in log])
    first = run(q)
    bad = dict(q)
    bad[where] = q[where].copy()
    bad[where][len(bad[where]) // 3, 0] = 1e9
    with pytest.raises(_lib.O3DMIError) as e:
        run(bad)
    assert e.value.status == KEY_RANGE, str(e.value)
    assert run(q) == first


_FORMS_SCRIPT = r"""
import sys, json
import numpy as np, torch
sys.path.insert(0, %(root)r)
from open3d_amd import registration as reg
out = []
for ns, nt, dt, voxels, md in %(rows)r:
    src = torch.from_numpy(np.load(%(dir)r + "/source_%%s.npy" %% dt)[:ns]).cuda()
    tgt = torch.from_numpy(np.load(%(dir)r + "/target_%%s.npy" %% dt)[:nt]).cuda()
    nrm = torch.from_numpy(
        np.load(%(dir)r + "/target_normals_%%s.npy" %% dt)[:nt]).cuda()
    crit = [reg.ICPConvergenceCriteria(1e-6, 1e-6, 6)] * len(voxels)
    log = []
    r = reg.multi_scale_icp(src, tgt, nrm, voxels, crit, md,
                            callback_after_iteration=log.append)
    out.append([r.transformation.tobytes().hex(), r.num_iterations,
                repr(r.fitness), repr(r.inlier_rmse),
                [[e["scale_index"], repr(e["fitness"]), repr(e["inlier_rmse"])]
                 for e in log]])
print(json.dumps(out))
"""


def test_pyramid_forms_agree_across_the_tiled_limit(clouds, tmp_path):
    """The mixed pairs and the both-sort pair under the default pyramid
    (paired, fused next-level inserts, counts posted by the coarsest reduce
    launch), as two chains on two streams (O3DMI_VDS_UNPAIRED=1), with the
    separate posting launch (O3DMI_VDS_POST_LAUNCH=1) and with an insert
    launch per level (O3DMI_VDS_NO_FUSE=1): every iteration's fitness and
    rmse, the pose, fitness and iteration count are the same bits. A fresh
    child process per setting (the settings are read once)."""
    _gpu()
    rows = [(N, N + 1, "float32", VS3, MD3),
            (N + 1, N, "float64", VS3, MD3),
            (900_000, 1_200_000, "float64", VS4, MD4),
            (1_200_000, 1_100_000, "float32", VS3, MD3)]
    for dt in (np.float32, np.float64):
        p = clouds(dt)
        m = 1_200_000
        for k in ("source", "target", "target_normals"):
            np.save(str(tmp_path / ("%s_%s.npy" % (k, np.dtype(dt).name))),
                    p[k][:m])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _FORMS_SCRIPT % {"root": root, "rows": rows,
                              "dir": str(tmp_path)}

    def run(env_extra):
        env = dict(os.environ)
        for k in ("O3DMI_VDS_UNPAIRED", "O3DMI_VDS_NO_FUSE",
                  "O3DMI_VDS_POST_LAUNCH"):
            env.pop(k, None)
        env.update(env_extra)
        r = subprocess.run([sys.executable, "-c", script], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    default = run({})
    assert len(default) == len(rows)
    for case, (ns, nt, dt, voxels, md) in zip(default, rows):
        assert case[1] > 0
        assert sorted(set(e[0] for e in case[4])) == list(range(len(voxels)))
    assert run({"O3DMI_VDS_UNPAIRED": "1"}) == default
    assert run({"O3DMI_VDS_POST_LAUNCH": "1"}) == default
    assert run({"O3DMI_VDS_NO_FUSE": "1"}) == default


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_down_sample_sort_form_with_normals(clouds, dtype):
    """Stand-alone VoxelDownSample beyond the tiled form (2^20 + 1 and 1.5 M
    points) with normals, chained over two levels as the pyramid does (the
    second level's input is the first one's output): the same bits as the
    oracle."""
    _lib, reg = _gpu()
    p = clouds(dtype)
    for n in (N + 1, BIG):
        pts = np.ascontiguousarray(p["target"][:n])
        nrm = np.ascontiguousarray(p["target_normals"][:n])
        for voxel in (0.0125, 0.05):
            wp, wn = orc.voxel_down_sample(pts, nrm, voxel)
            gp, gn = reg.voxel_down_sample(_dev(pts), _dev(nrm), voxel)
            assert gp.shape[0] == wp.shape[0]
            assert 1000 < wp.shape[0] < pts.shape[0]
            assert np.array_equal(gp.cpu().numpy(), wp)
            assert np.array_equal(gn.cpu().numpy(), wn)
            pts, nrm = wp, wn


def test_workspaces_across_a_grow_and_between_the_two_entry_points(clouds):
    """The VoxelDownSample workspaces live per host thread, device and chain,
    grow with the largest cloud seen, and chain 0's are shared by
    MultiScaleICP and the public voxel_down_sample. On a fresh host thread
    (fresh workspaces, whatever ran before): 3 000-point clouds allocate the
    first capacity (16 384 points, 2^15 table slots in use), 40 000-point
    clouds grow and re-initialise the used workspace (2^17 slots), the public
    entry then runs on it, and the small pair reuses the grown tables under
    its smaller mask. The second round of the same calls finds every table
    as clean as the first round did: the same bits. The down-sampled cloud
    is the oracle's, bit for bit."""
    _lib, reg = _gpu()
    p = clouds(np.float32)
    small, large = _problem(p, 3_000, 3_000), _problem(p, 40_000, 40_000)
    device = torch.cuda.current_device()

    def icp(q):
        r, log = _hip(reg, q, VS3, CRIT3, MD3, "plane")
        assert r.num_iterations > 0 and r.fitness > 0
        return (r.transformation.tobytes(), r.num_iterations, r.fitness,
                r.inlier_rmse, [(e["scale_index"], e["fitness"],
                                 e["inlier_rmse"]) for e in log])

    def down():
        gp, gn = reg.voxel_down_sample(_dev(large["target"]),
                                       _dev(large["target_normals"]), VS3[0])
        return gp.cpu().numpy(), gn.cpu().numpy()

    rounds, failure = [], []

    def sequence():
        try:
            torch.cuda.set_device(device)
            for _ in range(2):
                rounds.append((icp(small), icp(large), down()))
        except BaseException as e:  # reported by the test's own thread
            failure.append(e)
    t = threading.Thread(target=sequence)
    t.start()
    t.join()
    if failure:
        raise failure[0]
    (small_1, large_1, down_1), (small_2, large_2, down_2) = rounds
    assert small_2 == small_1
    assert large_2 == large_1
    assert down_2[0].shape == down_1[0].shape
    assert np.array_equal(down_2[0], down_1[0])
    assert np.array_equal(down_2[1], down_1[1])
    wp, wn = orc.voxel_down_sample(large["target"], large["target_normals"],
                                   VS3[0])
    assert 100 < wp.shape[0] < 40_000
    assert down_1[0].shape[0] == wp.shape[0]
    assert np.array_equal(down_1[0], wp)
    assert np.array_equal(down_1[1], wn)
