"""The numpy Doppler ICP oracle (_doppler_oracle.py) pinned before anything is
compared with it: against _oracle's point-to-plane accumulate (itself pinned to
the reference), against pose_to_transformation, and against the estimator's
purpose. No GPU."""
import numpy as np
import pytest

import _doppler_oracle as dop
import _oracle as orc
import test_oracle_goldens as G


def test_transformation_to_pose_inverts_pose_to_transformation():
    """(a) seeded poses with |beta| < 1.5, rtol 1e-12."""
    rng = np.random.default_rng(11)
    for _ in range(200):
        pose = np.concatenate([rng.uniform(-3.1, 3.1, 1),
                               rng.uniform(-1.5, 1.5, 1),
                               rng.uniform(-3.1, 3.1, 1),
                               rng.uniform(-5, 5, 3)])
        T = orc.pose_to_transformation(pose)
        np.testing.assert_allclose(dop.transformation_to_pose(T), pose,
                                   rtol=1e-12, atol=0)


def test_transformation_to_pose_gimbal_branch_by_hand():
    """sy < 1e-6 (beta = pi/2 exactly: R[0][0] = R[1][0] = 0): alpha =
    atan2(-R[1][2], R[1][1]), beta = atan2(-R[2][0], sy), gamma = 0."""
    a = 0.3
    T = np.eye(4)
    # Ry(pi/2) Rx(a) written out: rows (0, sin a, cos a), (0, cos a, -sin a),
    # (-1, 0, 0)
    T[:3, :3] = [[0, np.sin(a), np.cos(a)], [0, np.cos(a), -np.sin(a)],
                 [-1, 0, 0]]
    T[:3, 3] = [1, 2, 3]
    pose = dop.transformation_to_pose(T)
    np.testing.assert_allclose(pose, [a, np.pi / 2, 0, 1, 2, 3], rtol=1e-15)
    # and the pose gives the matrix back
    np.testing.assert_allclose(orc.pose_to_transformation(pose), T, atol=1e-15)


def _golden(dtype):
    n = G.SRC.shape[0]
    rng = np.random.default_rng(2)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (G.SRC.astype(dtype), rng.standard_normal(n).astype(dtype),
            d.astype(dtype), G.TGT.astype(dtype), G.TGT_N.astype(dtype),
            G.CORR)


def _prep(dtype, T=None, V=None, period=0.1):
    rng = np.random.default_rng(5)
    if T is None:
        T = orc.pose_to_transformation(rng.uniform(-0.2, 0.2, 6))
    return dop.host_prepare(V, T, period, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lambda_zero_reduces_to_point_to_plane(dtype):
    """(b) lambda_doppler = 0, L2, no rejection: sqrt_lambda_geometric = 1 and
    every Doppler term is a (signed) zero, so sums 0..26 and 28 are
    point-to-plane's, bit for bit per pair; [27] differs by definition (squared
    here). The golden 14 / 11-point set of test_oracle_goldens.py."""
    src, dops, dirs, tgt, tn, corr = _golden(dtype)
    R, r, w, v = _prep(dtype)
    got = dop.accumulate(src, dops, dirs, tgt, tn, corr, R, r, w, v, 0.1,
                         False, 2.0, (0, 1, 1), (0, 1, 1), 0.0)
    want = orc.p2plane_accumulate(src, tgt, tn, corr, accumulate_double=True)
    # same per-pair values; the two float64 sums differ in order only
    np.testing.assert_allclose(got[:27], want[:27], rtol=1e-14, atol=0)
    assert got[28] == want[28] == 14
    A, _ = dop.pair_terms(src, dops, dirs, tgt, tn, corr, R, r, w, v, 0.1,
                          False, 2.0, (0, 1, 1), (0, 1, 1), 0.0)
    for i in range(14):
        one = np.full(14, -1, np.int64)
        one[i] = corr[i]
        w1 = orc.p2plane_accumulate(src, tgt, tn, one, accumulate_double=True)
        assert np.array_equal(A[i, :27].astype(np.float64), w1[:27]), i


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rejected_pair_adds_only_to_the_count(dtype):
    """(c) a pair over the threshold: exactly 0 in sums 0..27, 1 in sum 28."""
    src, dops, dirs, tgt, tn, corr = _golden(dtype)
    R, r, w, v = _prep(dtype)
    args = (src, dops, dirs, tgt, tn, corr, R, r, w, v, 0.1)
    A0, rej0 = dop.pair_terms(*args, False, 0.8, (0, 1, 1), (0, 1, 1), 0.01)
    A1, rej1 = dop.pair_terms(*args, True, 0.8, (0, 1, 1), (0, 1, 1), 0.01)
    assert not rej0.any() and 0 < rej1.sum() < 14
    assert np.all(A1[rej1, :28] == 0) and np.all(A1[rej1, 28] == 1)
    assert np.array_equal(A1[~rej1], A0[~rej1])
    assert np.all(A0[rej1, 27] > 0)
    s = dop.accumulate(*args, True, 0.8, (0, 1, 1), (0, 1, 1), 0.01)
    assert s[28] == 14


def test_kernels_switch_on_at_the_stated_iterations():
    """(d) before its minimum iteration a kernel is L2(1, 1); rejection is off
    before its own; and the driver restarts the index at every scale."""
    p = dict(dop.DEFAULTS, geometric_kernel=(dop.HUBER, 0.5, 1.0),
             doppler_kernel=(dop.TUKEY, 0.3, 1.0), reject_dynamic_outliers=True,
             geometric_robust_loss_min_iteration=1,
             doppler_robust_loss_min_iteration=3,
             outlier_rejection_min_iteration=2)
    l2 = (dop.L2, 1.0, 1.0)
    assert dop.kernels_at(0, p) == (l2, l2, False)
    assert dop.kernels_at(1, p) == (p["geometric_kernel"], l2, False)
    assert dop.kernels_at(2, p) == (p["geometric_kernel"], l2, True)
    assert dop.kernels_at(3, p) == (p["geometric_kernel"],
                                    p["doppler_kernel"], True)
    assert dop.kernels_at(2, dict(p, reject_dynamic_outliers=False))[2] is False
    s = dop.plane_scene(n=600)
    out = dop.multiscale_icp(
        s["source"], s["dopplers"], s["directions"], s["target"],
        s["target_normals"], [1.0, -1.0], [(0, 0, 4), (0, 0, 4)], [2.0, 1.0],
        params=p)
    assert out["num_iterations"] == 8
    for scale in out["kernels_used"]:
        assert scale == [dop.kernels_at(i, p) for i in range(4)]


def test_doppler_resolves_the_in_plane_motion_point_to_plane_cannot():
    """(e) a single plane, the sensor translating inside it by (0.30, 0.10) m,
    dopplers from the reference's prediction at the true motion
    (plane_scene, seed 5, 5000 points, Float64, from the identity). In-plane
    translation error left by the oracle's ICP: Doppler 1.2e-5 m (7
    iterations, converged), point-to-plane 0.183 m (12 iterations, converged:
    it has nothing to pull it along the plane)."""
    s = dop.plane_scene()
    err = {}
    for est in ("doppler", "plane"):
        out = dop.multiscale_icp(
            s["source"], s["dopplers"], s["directions"], s["target"],
            s["target_normals"], [-1.0], [s["criteria"]], [s["max_dist"]],
            estimation=est)
        err[est] = dop.in_plane_error(out["transformation"], s["T_gt"])
    print("in-plane error: doppler %.3g m, point-to-plane %.3g m"
          % (err["doppler"], err["plane"]))
    assert err["doppler"] < 0.1 * err["plane"]
    assert err["doppler"] < 1e-3


def test_dopplers_vanish_at_the_true_motion():
    """The scene's premise: with the current transformation at the truth the
    Doppler residual of every point is zero (to rounding)."""
    s = dop.plane_scene(n=300)
    R, r, w, v = dop.host_prepare(None, s["T_gt"], 0.1, np.float64)
    pred = dop.predicted_doppler(s["directions"], R, r, w, v)
    assert np.abs(pred - s["dopplers"]).max() == 0
    assert np.abs(s["dopplers"]).max() > 1.0   # ~3 m/s along the motion
