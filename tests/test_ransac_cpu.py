"""CPU checks of the RANSAC restatement (tests/_ransac_oracle.py) against
hand-computed cases, and of the new C ABI symbols / Python names."""
import ctypes
import math

import numpy as np

import _ransac_oracle as ro


def test_sample_function_by_hand():
    # seed 0, counter 1: the first output of splitmix64 seeded with 0,
    # 0xE220A8397B1DCDAF; times 1000, high 64 bits
    z = 0xE220A8397B1DCDAF
    assert z == 16294208416658607535
    assert ro.draw(0, 0, 0, 1000) == (z * 1000) >> 64 == 883
    # worked out step by step with Python integers
    assert ro.draw(0, 0, 1, 1000) == 431       # z = 7960286522194355700
    assert ro.draw(1, 0, 0, 1000) == 566       # z = 10451216379200822465
    assert ro.draw(12345, 7, 2, (1 << 20) + 7) == 1012620
    assert ro.draw(0, (1 << 40) + 5, 7, 3) == 1
    assert ro.draw((1 << 64) - 1, 99999, 0, 5000) == 4930
    # no modulo: always below n, draws may repeat inside an iteration
    s = ro.samples(3, 0, 2000, 3, 5)
    assert s.min() == 0 and s.max() == 4
    assert (s[:, 0] == s[:, 1]).any()


def test_edge_length_checker_thresholds():
    s = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], float)
    t = s.copy()
    t[1, 0] = 0.8        # edge 0-1: 1.0 against 0.8
    t[2] = [0, 1, 0]
    # dis_target 0.8 < dis_source 1.0 * thr fails for thr > 0.8; the other
    # edges (1 / 1 and sqrt2 / sqrt(1.64)) pass up to 0.9055
    assert ro.check_edge_length(s, t, 0.8)[0]            # at: '<' is strict
    assert ro.check_edge_length(s, t, 0.8 - 1e-9)[0]     # just under
    assert not ro.check_edge_length(s, t, 0.8 + 1e-9)[0]  # just over
    # symmetric in source / target
    assert not ro.check_edge_length(t, s, 0.8 + 1e-9)[0]
    ok, margin = ro.check_edge_length(s, t, 0.8)
    assert margin == 0.0


def test_distance_checker_thresholds():
    s = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], float)
    t = s + [0, 0, 0.5]
    R, tr = np.eye(3), np.zeros(3)
    assert ro.check_distance(s, t, R, tr, 0.5)[0]             # at: '>' strict
    assert ro.check_distance(s, t, R, tr, 0.5 + 1e-9)[0]
    assert not ro.check_distance(s, t, R, tr, 0.5 - 1e-9)[0]
    # the motion is applied to the source
    assert ro.check_distance(s, t, R, np.array([0, 0, 0.5]), 1e-12)[0]


def test_normal_checker_thresholds():
    a = 0.25
    sn = np.array([[0, 0, 1.0]] * 3)
    tn = np.array([[math.sin(a), 0, math.cos(a)]] * 3)
    R = np.eye(3)
    d = float(tn[0] @ sn[0])
    # passes iff dot >= cos(threshold)
    assert ro.check_normal(sn, tn, R, math.acos(d))[0] == \
        (not d < math.cos(math.acos(d)))
    assert ro.check_normal(sn, tn, R, a + 1e-6)[0]
    assert not ro.check_normal(sn, tn, R, a - 1e-6)[0]
    # a rotation of the source normals onto the target's passes any angle
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0],
                   [-math.sin(a), 0, math.cos(a)]])
    assert ro.check_normal(sn, tn, Ry, 1e-7)[0]
    # no normals on either side: passes
    assert ro.check_normal(None, tn, R, 0.0)[0]


def test_stopping_bound():
    # ratio 0: log(1) = 0 -> k = -inf: no exit
    assert ro.update_bound(100, 0.0, 3, 0.999) == 100
    # ratio 1: log(0) = -inf -> k = +0: exit at once
    assert ro.update_bound(100, 1.0, 3, 0.999) == 0
    # confidence 1.0: k = +inf (or NaN): never exit
    assert ro.update_bound(100, 0.5, 3, 1.0) == 100
    assert ro.update_bound(100, 1.0, 3, 1.0) == 100
    assert ro.update_bound(100, 0.0, 3, 1.0) == 100
    # log(0.001) / log(1 - 0.125) = 51.73 -> 52; never raises the bound
    assert ro.update_bound(100000, 0.5, 3, 0.999) == 52
    assert ro.update_bound(40, 0.5, 3, 0.999) == 40


def test_loop_tie_rule_and_bound():
    # iterations 2 and 5 tie on (fitness, rmse): the lower one stays; 7 wins
    # on rmse at equal fitness; rejected iterations are not validations
    scores = {2: (0.5, 0.1, 0.0), 5: (0.5, 0.1, 0.0), 7: (0.5, 0.05, 0.0),
              8: (0.4, 0.0, 0.0)}
    out = ro.loop(10, 3, 0.999, lambda i: i in scores, lambda i: scores[i])
    assert out["best_iteration"] == 7 and out["num_validations"] == 4
    assert out["final_iteration_bound"] == 10
    out = ro.loop(7, 3, 0.999, lambda i: i in scores, lambda i: scores[i])
    assert out["best_iteration"] == 2 and out["num_validations"] == 2
    # fitness 0 never becomes the best
    out = ro.loop(5, 3, 0.999, lambda i: True, lambda i: (0.0, 0.0, 0.0))
    assert out["best_iteration"] == -1 and out["num_validations"] == 5
    # iteration 1 moves the bound to 3: iterations 3.. do not take part, and
    # a rejected iteration cannot move it
    seen = []

    def score(i):
        seen.append(i)
        return (0.1 * (i + 1), 0.0, 0.97 if i == 1 else 0.0)
    out = ro.loop(100, 3, 0.999, lambda i: i != 0, score)
    assert ro.update_bound(100, 0.97, 3, 0.999) == 3
    assert seen == [1, 2] and out["final_iteration_bound"] == 3
    assert out["best_iteration"] == 2 and out["num_validations"] == 2


def test_hypothesis_recovers_motion_and_rejects_degenerate():
    rng = np.random.RandomState(0)
    src = rng.uniform(-1, 1, (50, 3))
    a = 0.4
    R = np.array([[math.cos(a), -math.sin(a), 0],
                  [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    tgt = src @ R.T + [0.1, 0.2, -0.3]
    corres = np.stack([np.arange(50), np.arange(50)], 1)
    h = ro.hypothesis(src, tgt, corres, [3, 17, 40],
                      [(ro.EDGE, 0.9), (ro.DISTANCE, 1e-9)])
    assert h["passed"]
    assert np.abs(h["T"][:3, :3] - R).max() < 1e-12
    assert np.abs(h["T"][:3, 3] - [0.1, 0.2, -0.3]).max() < 1e-12
    # a repeated pair: rank one
    assert not ro.hypothesis(src, tgt, corres, [3, 3, 40])["passed"]


def test_batch_schedule_never_exceeds_the_round_buffers():
    """The driver sizes every per-round buffer by the cap of its batch
    schedule (2^22 (survivor, tile) partials, 16384 hypotheses): whatever the
    rounds report, no batch may exceed it -- in particular for clouds of more
    than 2^24 points, whose cap lies below the schedule's floor of 64."""
    from open3d_amd import _lib
    import __graft_entry__ as ge
    ge.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    f = so.o3dmi_internal_ransac_next_batch
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_int64)]
    cap = ctypes.c_int64(0)
    for ns, want_cap in ((5000, 16384), (20000, 16384), (1 << 20, 1024),
                         ((1 << 24) + 1, 63), (1 << 26, 16), (1 << 31, 1)):
        tiles = (ns + 255) // 256
        f(1, ns, 0, ctypes.byref(cap))
        assert cap.value == want_cap == max(1, min(16384, (1 << 22) // tiles))
        batch = min(1024, cap.value)
        for n_surv in (0, 1, 7, 10 ** 6, 0, 0, 0, 0, 0, 10 ** 9, 10 ** 9, 10 ** 9,
                       10 ** 9, 10 ** 9, 10 ** 9, 10 ** 9, 10 ** 9, 3, 0):
            nxt = f(batch, ns, n_surv, None)
            assert 1 <= nxt <= cap.value, (ns, batch, n_surv, nxt)
            q = max(n_surv, 1) * ns
            if q < (1 << 21):
                assert nxt == min(2 * batch, cap.value)
            elif q > (1 << 24):
                assert nxt == min(max(batch // 2, 64), cap.value)
            else:
                assert nxt == batch
            batch = nxt


def test_ransac_symbols_exported():
    from open3d_amd import _lib, registration
    import __graft_entry__ as ge
    ge.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    for name in ("o3dmi_ransac_hypotheses", "o3dmi_ransac_score",
                 "o3dmi_ransac_score_scratch_bytes",
                 "o3dmi_registration_ransac_correspondence",
                 "o3dmi_registration_ransac_feature_matching"):
        assert hasattr(so, name), name
        assert name in _lib.PROTOTYPES, name
    for name in ("RANSACConvergenceCriteria",
                 "CorrespondenceCheckerBasedOnEdgeLength",
                 "CorrespondenceCheckerBasedOnDistance",
                 "CorrespondenceCheckerBasedOnNormal",
                 "registration_ransac_based_on_correspondence",
                 "registration_ransac_based_on_feature_matching"):
        assert hasattr(registration, name), name
    c = registration.RANSACConvergenceCriteria()
    assert c.max_iteration == 100000 and c.confidence == 0.999
