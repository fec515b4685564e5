"""CPU checks of the Fast Global Registration restatement
(tests/_fgr_oracle.py) on the standard scene, and of the new C ABI symbols /
Python names.

Standard scene (fo.scene): 300 (or 1000) source points uniform in a
2 x 1.4 x 0.8 box about the origin, the target the source under a rotation of
1.3 rad plus a translation, Gaussian noise 0.002, shuffled rows; one pair per
source row, a stated share of them with a random target row.

Pose bound: 5e-3 rad and 5e-3 against ground truth. With noise 0.002 the
restatement lands between 0.3e-3 and 3.2e-3 over seeds 1-6; the bound guards
convergence, not rounding.

Recorded on this restatement (seeds below): d, the largest change of the result
over 8 random permutations of the correspondence rows, is 4.3e-16 (Frobenius
norm of the 3x3 difference) / 5.8e-16 (translation); the tile tree against a
plain sequential sum of the same terms moves the result by 3.4e-16 / 5.6e-17."""
import ctypes
import math

import numpy as np
import pytest

import _fgr_oracle as fo
import _ransac_oracle as ro

BOUND_RAD = 5e-3
BOUND_T = 5e-3
# (points, share of random pairs, seed)
CASES = {"50": (300, 0.5, 1), "70": (300, 0.7, 2), "80": (1000, 0.8, 3)}


@pytest.fixture(scope="module")
def scenes():
    return {k: fo.scene(*v) for k, v in CASES.items()}


def test_tile_tree_restatements_agree():
    rng = np.random.RandomState(0)
    rows = rng.normal(size=(700, 5)) * 10.0 ** rng.randint(-6, 6, (700, 5))
    t = fo.tile_sums(rows)
    assert t.shape == (3, 5)
    for k in range(3):
        assert np.array_equal(fo.tile_sum_plain(rows[256 * k:256 * (k + 1)]),
                              t[k])
    # a short tile: the missing rows add +0.0
    assert np.array_equal(fo.tile_sums(rows[:1])[0], rows[0])
    # levels: 70000 rows -> 274 tiles -> 2 -> 1
    big = rng.normal(size=(70000, 3))
    lv = fo.sum_levels(big)
    assert np.array_equal(lv, fo.tile_sums(fo.tile_sums(fo.tile_sums(big)))[0])
    assert np.abs(lv - big.sum(0)).max() < 1e-9
    # tile order: sequential over the tile sums
    s = fo.sum_tiles_in_order(rows)
    assert np.array_equal(s, (t[0] + t[1]) + t[2])


def test_draws_equal_the_ransac_sample_function():
    for seed, n in ((0, 300), (5, 3), ((1 << 64) - 1, 99991)):
        want = ro.samples(seed, 0, 500, 3, n)
        got = np.array([[fo.draw(seed, t, j, n) for j in range(3)]
                        for t in range(500)], np.int64)
        assert np.array_equal(got, want)
    assert fo.draw(0, 0, 0, 1000) == 883  # the RANSAC test's hand value


def test_pose_recovered_without_tuple_test(scenes):
    for k in ("50", "70", "80"):
        src, tgt, corres, T = scenes[k]
        got, info = fo.fgr_correspondence(src, tgt, corres, tuple_test=False)
        ang, tr = fo.pose_error(got, T)
        print("no tuple test, %s %% random: %.2e rad / %.2e" % (k, ang, tr))
        assert ang < BOUND_RAD and tr < BOUND_T
        assert info["n_used"] == len(corres) and info["failed_solves"] == 0
        # par: scale_global / 1.4 every fourth iteration while above 0.025
        par = info["scale_global"]
        for itr in range(64):
            if itr % 4 == 0 and par > 0.025:
                par = par / 1.4
        assert info["final_par"] == par


def test_tuple_test_both_branches_and_pose(scenes):
    # 50 % random: the cap of 1000 tuples is reached early
    src, tgt, corres, T = scenes["50"]
    got, info = fo.fgr_correspondence(src, tgt, corres, seed=1)
    assert info["n_tuples"] == 1000 and info["n_trials"] < 100 * len(corres)
    assert info["n_used"] == 3000
    true = {(int(a), int(b)) for a, b in corres
            if np.linalg.norm(src[a] @ T[:3, :3].T + T[:3, 3] - tgt[b]) < 0.02}
    share = np.mean([(int(a), int(b)) in true for a, b in info["used"]])
    print("50 %% random: cap at trial %d, %.1f %% of kept pairs true" %
          (info["n_trials"], 100 * share))
    assert share > 0.9
    ang, tr = fo.pose_error(got, T)
    assert ang < BOUND_RAD and tr < BOUND_T
    # 70 % random: all 100 * ncorr trials run, below the cap
    src, tgt, corres, T = scenes["70"]
    got, info = fo.fgr_correspondence(src, tgt, corres, seed=2)
    assert info["n_trials"] == 100 * len(corres) == 30000
    assert 0 < info["n_tuples"] < 1000
    assert info["n_used"] == 3 * info["n_tuples"]
    print("70 %% random: %d tuples" % info["n_tuples"])
    ang, tr = fo.pose_error(got, T)
    assert ang < BOUND_RAD and tr < BOUND_T


def test_tuple_test_early_exit_is_the_sequential_loop(scenes):
    src, tgt, corres, _ = scenes["50"]
    full, n_full, trials_full = fo.tuple_test(src, tgt, corres, 0.95, 10 ** 9,
                                              7)
    assert trials_full == 100 * len(corres) and len(full) == 3 * n_full
    for cap in (1, 17, n_full):
        t, n, trials = fo.tuple_test(src, tgt, corres, 0.95, cap, 7)
        assert n == cap and np.array_equal(t, full[:3 * cap])
        assert trials <= trials_full
    # the kept pairs are rows of corres, three per tuple in draw order
    t, n, trials = fo.tuple_test(src, tgt, corres, 0.95, 1, 7)
    r = [fo.draw(7, trials - 1, j, len(corres)) for j in range(3)]
    assert np.array_equal(t, corres[r])
    # ncorr <= 2: no tuples, no trials
    for m in (0, 1, 2):
        t, n, trials = fo.tuple_test(src, tgt, corres[:m], 0.95, 1000, 0)
        assert t.shape == (0, 2) and n == 0 and trials == 0


def test_permuting_the_correspondences_moves_the_result_by_rounding(scenes):
    src, tgt, corres, _ = scenes["50"]
    base, _ = fo.fgr_correspondence(src, tgt, corres, tuple_test=False)
    rng = np.random.RandomState(11)
    d_rot = d_tr = 0.0
    for _ in range(8):
        got, _ = fo.fgr_correspondence(src, tgt,
                                       corres[rng.permutation(len(corres))],
                                       tuple_test=False)
        a, b = fo.pose_change(got, base)
        d_rot, d_tr = max(d_rot, a), max(d_tr, b)
    print("d over 8 permutations: %.2e (Frobenius) / %.2e (translation)" %
          (d_rot, d_tr))
    # recorded, and far below what a wrong order of operations would give
    assert d_rot < 1e-12 and d_tr < 1e-12
    # the tile tree against upstream's sequential sum: rounding only
    nrm = fo.normalize(src, tgt)
    a = fo.optimize(nrm["clouds"][0], nrm["clouds"][1], corres,
                    nrm["scale_global"])[0]
    b = fo.optimize(nrm["clouds"][0], nrm["clouds"][1], corres,
                    nrm["scale_global"], order="sequential")[0]
    e = fo.pose_change(a, b)
    print("tile tree against a sequential sum: %.2e / %.2e" % e)
    assert e[0] < 1e-12 and e[1] < 1e-12


def test_fewer_than_ten_pairs_gives_the_mean_shift(scenes):
    src, tgt, corres, _ = scenes["50"]
    got, info = fo.fgr_correspondence(src, tgt, corres[:9], tuple_test=False)
    want = np.eye(4)
    # inverse of [I | mean_source - mean_target]
    want[:3, 3] = -(fo.sum_levels(src) / 300.0 - fo.sum_levels(tgt) / 300.0)
    assert np.array_equal(got, want) and info["failed_solves"] == 0
    # no iteration: the same
    got0, _ = fo.fgr_correspondence(src, tgt, corres, tuple_test=False,
                                    iteration_number=0)
    assert np.array_equal(got0, want)
    # ncorr <= 2 with the tuple test: no tuples, so the identity path
    got2, info2 = fo.fgr_correspondence(src, tgt, corres[:2])
    assert info2["n_tuples"] == 0 and info2["n_used"] == 0
    assert np.array_equal(got2, want)


def test_solve_and_rotation_by_hand():
    # Rz(c) Ry(b) Rx(a) against the product of the three matrices
    a, b, c = 0.3, -0.7, 1.9
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)],
                   [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0],
                   [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0],
                   [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    T = fo.vector6_to_matrix([a, b, c, 1.0, 2.0, 3.0])
    assert np.abs(T[:3, :3] - Rz @ Ry @ Rx).max() < 1e-15
    assert np.array_equal(T[:3, 3], [1.0, 2.0, 3.0])
    # the solve against numpy on a well-conditioned system
    rng = np.random.RandomState(2)
    M = rng.normal(size=(6, 6))
    A = M @ M.T + 6 * np.eye(6)
    rhs = rng.normal(size=6)
    x = fo.solve(A, rhs)
    assert np.abs(np.array(x) - np.linalg.solve(-A, rhs)).max() < 1e-13
    # a pivot that is not positive: no solution
    A[2, 2] = -1.0
    assert fo.solve(A, rhs) is None
    assert fo.solve(np.zeros((6, 6)), rhs) is None
    # all pairs one point on the z axis with p == q: JTJ is exactly singular
    p = np.tile([[0.0, 0.0, 1.0]], (64, 1))
    trans, par, failed = fo.optimize(p, p, np.zeros((64, 2), np.int64), 1.0,
                                     iteration_number=5)
    assert failed == 5 and np.array_equal(trans, np.eye(4))


def test_terms_match_the_reference_loop_shape():
    # the 27 numbers of one correspondence from the rows as upstream writes
    # them (J J^T s and J r s, row by row)
    p = np.array([[0.3, -0.2, 0.5]])
    q = np.array([[0.1, 0.4, -0.6]])
    par = 0.7
    r = p[0] - q[0]
    s = (par / (r @ r + par)) ** 2
    J = np.array([[0, -q[0, 2], q[0, 1], -1, 0, 0],
                  [q[0, 2], 0, -q[0, 0], 0, -1, 0],
                  [-q[0, 1], q[0, 0], 0, 0, 0, -1]], float)
    JTJ = sum(np.outer(J[k], J[k]) * s for k in range(3))
    JTr = sum(J[k] * r[k] * s for k in range(3))
    t = fo.terms(p, q, par)[0]
    iu = np.triu_indices(6)
    assert np.abs(t[:21] - JTJ[iu]).max() < 1e-15
    assert np.abs(t[21:] - JTr).max() < 1e-15


def test_fgr_symbols_exported():
    from open3d_amd import _lib, registration
    import __graft_entry__ as ge
    ge.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    for name in ("o3dmi_fgr_tuple_test", "o3dmi_fgr_optimize",
                 "o3dmi_fgr_optimize_scratch_bytes",
                 "o3dmi_registration_fgr_correspondence",
                 "o3dmi_registration_fgr_feature_matching"):
        assert hasattr(so, name), name
        assert name in _lib.PROTOTYPES, name
    for name in ("o3dmi_internal_fgr_tuple_test",
                 "o3dmi_internal_fgr_optimize",
                 "o3dmi_internal_fgr_stream_scratch_bytes",
                 "o3dmi_internal_fgr_resident_capacity"):
        assert hasattr(so, name), name
        assert name in _lib.INTERNAL_PROTOTYPES, name
    f = so.o3dmi_internal_fgr_resident_capacity
    f.restype = ctypes.c_int64
    assert f() == 4096
    g = so.o3dmi_fgr_optimize_scratch_bytes
    g.restype = ctypes.c_size_t
    g.argtypes = [ctypes.c_int64]
    assert g(4096) == 0 and g(4097) > 48 * 4097
    for name in ("FastGlobalRegistrationOption",
                 "registration_fgr_based_on_correspondence",
                 "registration_fgr_based_on_feature_matching"):
        assert hasattr(registration, name), name
    o = registration.FastGlobalRegistrationOption()
    assert (o.division_factor, o.use_absolute_scale, o.decrease_mu,
            o.maximum_correspondence_distance, o.iteration_number,
            o.tuple_scale, o.maximum_tuple_count, o.tuple_test, o.seed) == \
        (1.4, False, True, 0.025, 64, 0.95, 1000, True, 0)
    assert ctypes.sizeof(_lib.FgrOptionsC) == 56
    assert ctypes.sizeof(_lib.FgrInfoC) == 64
