"""The numpy restatement of the rigid multiway optimizer (tests/_slac_oracle.py)
checked on its own: block structure, a known answer, the pruning rule and
convergence on the test scene. No GPU."""
import functools

import numpy as np

import _slac_oracle as so

F = np.float32


def _random_pairs(m, seed):
    rng = np.random.RandomState(seed)
    p = rng.uniform(-1, 1, (m, 3)).astype(F)
    q = (p + rng.normal(0, 0.03, (m, 3))).astype(F)
    n = rng.normal(size=(m, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    return p, q, n


def test_block_structure_is_exact():
    """The reference's 12-Jacobian (J, -J) gives [[A, -A], [-A, A]] and
    [b, -b] exactly: float32 products commute and (-x)(-y) = xy, (-x)y = -(xy)
    bit for bit, and the sums here are exactly rounded."""
    p, q, n = _random_pairs(5000, 1)
    thr = 0.02
    take, terms, _, _ = so.pair_terms(p, q, n, thr)
    assert 0 < take.sum() < take.size  # both sides of the threshold occur
    A12, b12, res = so.full_block(p, q, n, thr)
    cA, cb, cres = so.compact_block(so.exact_sums(take, terms))
    assert np.array_equal(A12, cA)
    assert np.array_equal(b12, cb)
    assert res == cres


def test_threshold_is_strictly_greater():
    """|r| == threshold stays: the reference returns on abs(r) > threshold."""
    p = np.array([[0.5, 0, 0], [0.5, 0, 0], [0.5, 0, 0]], F)
    q = np.array([[0.25, 0, 0], [0.25, 0, 0], [0.125, 0, 0]], F)
    n = np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0]], F)
    take, _, _, r = so.pair_terms(p, q, n, 0.25)
    assert r.tolist() == [0.25, -0.25, 0.375]
    assert take.tolist() == [True, True, False]


def test_identical_fragments_identical_poses_do_not_move():
    pts, nrm = so.surface(4000, 3)
    frag = (pts.astype(F), nrm.astype(F))
    T = so._rigid(np.random.RandomState(2), 30.0, 0.4)
    r = so.rigid_optimize([frag, frag], [T, T], [(0, 1, np.eye(4))],
                          max_iterations=3)
    assert r["status"] == "ok" and r["kept"] == [True]
    assert r["n_corres"] == [4000] and r["n_inliers"] == [4000]
    assert r["losses"] == [0.0, 0.0, 0.0]
    for got in r["poses"]:
        assert np.array_equal(got, T)


def _two_clouds(offset):
    rng = np.random.RandomState(5)
    a = rng.uniform(-1, 1, (500, 3)).astype(F)
    b = (a + F(offset)).astype(F)
    return a, b


def test_pruning_rule_branches():
    a, b = _two_clouds(0.0)
    I = np.eye(4)
    far = np.eye(4)
    far[0, 3] = 5.0
    # T_ij matches every point, the node poses disagree completely: ratio 0
    odo = so.correspondence_set(a, b, 3, 4, I, far, I, 0.07, 0.3)
    assert odo["corres"].shape[0] == 500 and odo["inliers"] == 0
    assert odo["ratio"] == 0 and odo["kept"]          # j == i + 1: kept
    loop = so.correspondence_set(a, b, 3, 5, I, far, I, 0.07, 0.3)
    assert loop["ratio"] == 0 and not loop["kept"]    # j != i + 1: dropped
    back = so.correspondence_set(a, b, 4, 3, I, far, I, 0.07, 0.3)
    assert not back["kept"]                           # j == i - 1 is a loop
    good = so.correspondence_set(a, b, 3, 5, I, I, I, 0.07, 0.3)
    assert good["ratio"] == 1 and good["kept"]
    # nothing within the radius: C == 0, dropped even as an odometry edge
    none = so.correspondence_set(a, b, 3, 4, I, I, far, 0.07, 0.3)
    assert none["corres"].shape[0] == 0 and not none["kept"]
    assert np.isnan(none["ratio"])


def test_inlier_test_is_less_or_equal_at_d_squared():
    d = F(0.25)
    p = np.zeros((2, 3), F)
    p[1, 1] = 10.0
    q = np.array([[0.25, 0, 0], [np.nextafter(F(0.25), F(1)), 10, 0]], F)
    T_ij = np.eye(4)
    T_ij[0, 3] = 0.25  # the search sees both pairs at distance ~0
    r = so.correspondence_set(p, q, 0, 1, np.eye(4), np.eye(4), T_ij, d, 0.3)
    assert r["corres"].tolist() == [[0, 0], [1, 1]]
    # |p0 - q0|^2 == d * d exactly: an inlier; the next float up is not
    assert r["inliers"] == 1 and r["ratio"] == F(0.5)


@functools.lru_cache(maxsize=None)
def scene_run():
    frags, truth, start, edges = so.make_scene()
    return frags, truth, start, edges, so.rigid_optimize(frags, start, edges)


def test_scene_inputs_are_well_conditioned():
    frags, _, _, edges, r = scene_run()
    assert all(20000 <= f[0].shape[0] <= 40000 for f in frags)
    assert r["kept"] == [True] * len(edges)
    assert min(r["n_corres"]) >= 1000
    reached = {0}
    for _ in range(len(frags)):
        for (i, j, _), k in zip(edges, r["kept"]):
            if k and (i in reached or j in reached):
                reached |= {i, j}
    assert reached == set(range(len(frags)))


def test_restatement_converges_on_the_scene():
    """5 fragments of ~33 k points, poses perturbed by up to 2 degrees / 3 cm,
    4 odometry + 2 loop edges with the true T_ij, upstream's defaults.
    Measured (rotation degrees, translation) of T_0^-1 T_k, before -> after 5
    iterations:
        k=1  0.776, 0.0375 -> 0.0075, 0.00026   (103x, 144x)
        k=2  0.593, 0.0242 -> 0.0188, 0.00061   ( 32x,  40x)
        k=3  2.988, 0.0291 -> 0.0245, 0.00034   (122x,  85x)
        k=4  2.885, 0.0632 -> 0.0214, 0.00047   (135x, 133x)
    loss 46.96, 0.0881, 0.0565, 0.0565, 0.0565. The assertion is the issue's
    after <= before / 2 per node (the measured run has a factor 15 to spare)."""
    _, truth, start, _, r = scene_run()
    assert r["status"] == "ok"
    before = so.relative_errors(start, truth)
    after = so.relative_errors(r["poses"], truth)
    for k, (b, a) in enumerate(zip(before, after), 1):
        print("node %d: %.4f deg %.5f -> %.4f deg %.5f" % ((k,) + b + a))
        assert a[0] <= b[0] / 2 and a[1] <= b[1] / 2, (k, b, a)
    assert r["losses"][-1] < r["losses"][0]


def test_solve_lu_matches_numpy_and_flags_singular():
    rng = np.random.RandomState(0)
    A = rng.normal(size=(30, 30))
    A = A @ A.T + np.eye(30)
    b = rng.normal(size=30)
    assert np.allclose(so.solve_lu(A, b), np.linalg.solve(A, b), rtol=1e-9)
    A[:, 7] = 0
    A[7, :] = 0
    assert so.solve_lu(A, b) is None


def test_new_entry_points_are_declared_and_bound():
    """Every symbol of the feature is in a public header and in the ctypes
    table (tests/test_abi.py then checks export without a GPU)."""
    import os

    from open3d_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kernel_h = open(os.path.join(root, "include", "o3d_mi355x.h")).read()
    host_h = open(os.path.join(root, "include", "o3d_mi355x_host.h")).read()
    for name in ("o3dmi_fill_in_rigid_alignment_term",
                 "o3dmi_slac_rigid_terms"):
        assert name + "(" in kernel_h and name in _lib.PROTOTYPES
    for name in ("o3dmi_slac_correspondence_set",
                 "o3dmi_slac_rigid_optimize"):
        assert name + "(" in host_h and name in _lib.PROTOTYPES
