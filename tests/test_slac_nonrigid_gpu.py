"""The non-rigid SLAC optimizer on the MI355X against the numpy restatement
(tests/_slac_nonrigid_oracle.py): the alignment seam, the regularizer seam,
the SPD solver and the whole optimizer."""
import numpy as np
import pytest
import torch

import _control_grid_oracle as cg
import _slac_nonrigid_oracle as no
import _slac_oracle as so
from _slac_nonrigid_oracle import (ALL_KEYS, GRID_SIZE, N_FRAGS, N_VARS, SIDE,
                                   oracle_run, regularizer_cases, scene,
                                   seam_inputs)

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, SINGULAR, UNSUPPORTED = 1, 5, 7
PANEL = 32                                # kSlacCholPanel
EPS = 2.0 ** -52

# Largest deviations from the float64 oracle measured on the MI355X with these
# inputs (recorded in profiles/slac_nonrigid_bench.json); the tests assert
# 16 x these.
REG_DEVIATION = 3.57e-8     # regularizer seam, relative to the largest entry
# The driver against the oracle driver with the library's gauge (pin_anchor:
# the reference's system is singular, _slac_nonrigid_oracle.slac_optimize),
# three iterations. Measured on the MI355X: poses 1.11e-14 (asserted at 16 x);
# nodes and all three losses measured 0, so their bounds come from the number
# formats instead. Both sides add the same float32 terms in another float64
# order, so x agrees to rounding and a node (float32, below 4 m) may land on
# the neighbouring float32, 2^-22 m, twice for safety. The first loss is the
# same 6625 terms in another order (count x 2^-52); later ones see nodes
# 2^-21 off, which moves a residual by at most that against an rms residual
# of sqrt(0.023 / 6625) = 1.9e-3: 2 x 2^-21 / 1.9e-3 relative.
DRIVER_POSE_DEVIATION = 1.11e-14    # |pose - oracle pose|, entrywise, measured
NODE_BOUND = 2.0 ** -21             # |node - oracle node|, metres
LOSS_BOUNDS = (6625 * 2.0 ** -52, 2 * 2.0 ** -21 / 1.9e-3,
               2 * 2.0 ** -21 / 1.9e-3)  # relative, per iteration


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_alignment_seam(arrays, threshold, i=1, j=2, n_vars=N_VARS, prev=None):
    from open3d_amd import slac
    AtA = torch.zeros((n_vars, n_vars), dtype=torch.float32, device="cuda")
    Atb = torch.zeros(n_vars, dtype=torch.float32, device="cuda")
    res = torch.zeros(1, dtype=torch.float32, device="cuda")
    if prev is not None:
        AtA += _cuda(prev[0])
        Atb += _cuda(prev[1])
        res += _cuda(prev[2])
    st = slac.fill_in_slac_alignment_term_raw(
        AtA, Atb, res, *[_cuda(a) for a in arrays], i, j, N_FRAGS, threshold)
    return st, AtA.cpu().numpy(), Atb.cpu().numpy(), res.cpu().numpy()


def _within(got, exact, mag, cnt, what):
    """exact - bound <= the float64 sum <= exact + bound with bound = count x
    2^-52 x sum |terms| (float64 summation in any order); the seam returns the
    float32 rounding of that sum, and rounding is monotonic."""
    bound = cnt * EPS * mag
    lo, hi = (exact - bound).astype(F), (exact + bound).astype(F)
    bad = ~((got >= lo) & (got <= hi))
    worst = np.abs(got.astype(np.float64) - exact) / np.maximum(mag, 1e-300)
    print("%s: worst |got - exact| / sum|terms| = %.3g" %
          (what, float(worst.max())))
    assert not bad.any(), (what, np.argwhere(bad)[:5])


@pytest.mark.parametrize("count", [1, 255, 1024, 1025, 2049])
def test_alignment_seam_matches_exact_sums(count):
    arrays = seam_inputs(count, 100 + count)
    take, J, idx, r = no.pair_jacobians(*arrays, 1, 2, N_FRAGS, 0.05)
    if count > 200:
        assert 0 < take.sum() < count      # both sides of the threshold
    want = no.exact_system(take, J, idx, r, N_VARS)
    st, A, b, res = run_alignment_seam(arrays, 0.05)
    assert st == 0
    _within(A, want["AtA"], want["mag_A"], want["cnt_A"], "AtA")
    _within(b, want["Atb"], want["mag_b"], want["cnt_b"], "Atb")
    _within(res, np.array([want["residual"]]), np.array([want["mag_r"]]),
            np.array([want["cnt_r"]]), "residual")
    assert np.array_equal(A, A.T)
    # the pose block and the residual are fixed trees: equal across runs
    st2, A2, b2, res2 = run_alignment_seam(arrays, 0.05)
    assert st2 == 0
    assert np.array_equal(A[:18, :18], A2[:18, :18])
    assert np.array_equal(b[:18], b2[:18]) and np.array_equal(res, res2)


def test_alignment_seam_dyadic_inputs_match_bit_for_bit():
    arrays = seam_inputs(1500, 5, dyadic=True)
    take, J, idx, r = no.pair_jacobians(*arrays, 1, 2, N_FRAGS, 0.0625)
    assert 0 < take.sum() < 1500
    want = no.exact_system(take, J, idx, r, N_VARS)
    for reverse in (False, True):
        A, b, res = no.naive_system(take, J, idx, r, N_VARS, reverse)
        assert np.array_equal(A, want["AtA"]) and np.array_equal(
            b, want["Atb"]) and res == want["residual"]
    runs = [run_alignment_seam(arrays, 0.0625) for _ in range(2)]
    for st, A, b, res in runs:
        assert st == 0
        assert np.array_equal(A, want["AtA"].astype(F))
        assert np.array_equal(b, want["Atb"].astype(F))
        assert res[0] == F(want["residual"])


def test_alignment_seam_adds_to_what_is_there():
    arrays = seam_inputs(300, 9)
    rng = np.random.RandomState(1)
    prev = (rng.normal(size=(N_VARS, N_VARS)).astype(F),
            rng.normal(size=N_VARS).astype(F), np.array([3.0], F))
    _, A0, b0, r0 = run_alignment_seam(arrays, 0.05)
    st, A, b, res = run_alignment_seam(arrays, 0.05, prev=prev)
    assert st == 0
    # one rounding of the sum, one of the addition; entries without terms
    # are left as they were
    assert np.array_equal(A, (prev[0] + A0).astype(F))
    assert np.array_equal(b, (prev[1] + b0).astype(F))
    assert np.array_equal(res, (prev[2] + r0).astype(F))
    assert np.array_equal(A[A0 == 0], prev[0][A0 == 0])


def test_alignment_seam_keeps_r_equal_to_threshold():
    a = list(seam_inputs(3, 2, dyadic=True))
    a[1] = np.array([[1.25, 1, 1], [1.25, 1.5, 1], [1.25, 2, 1]], F)
    a[0] = a[1] + np.array([[0.25, 0, 0], [-0.25, 0, 0], [0.5, 0, 0]], F)
    a[3] = np.array([[1, 0, 0]] * 3, F)
    take, J, idx, r = no.pair_jacobians(*a, 1, 2, N_FRAGS, 0.25)
    assert take.tolist() == [True, True, False]
    want = no.exact_system(take, J, idx, r, N_VARS)
    st, A, b, res = run_alignment_seam(a, 0.25)
    assert st == 0 and res[0] == F(0.125)
    assert np.array_equal(A, want["AtA"].astype(F))


def test_alignment_seam_all_pairs_beyond_threshold_touch_nothing():
    arrays = seam_inputs(700, 3)
    rng = np.random.RandomState(2)
    prev = (rng.normal(size=(N_VARS, N_VARS)).astype(F),
            rng.normal(size=N_VARS).astype(F), np.array([2.5], F))
    take = no.pair_jacobians(*arrays, 1, 2, N_FRAGS, 1e-12)[0]
    assert not take.any()
    st, A, b, res = run_alignment_seam(arrays, 1e-12, prev=prev)
    assert st == 0
    for got, was in zip((A, b, res), prev):
        assert got.tobytes() == was.tobytes()


@pytest.mark.parametrize("where", ["p", "q", "negative"])
def test_alignment_seam_rejects_a_node_outside_the_system(where):
    a = list(seam_inputs(1500, 4))
    a[5], a[6] = a[5].copy(), a[6].copy()
    if where == "p":
        a[5][1200, 3] = SIDE ** 3          # 18 + 3 * 64 + 2 >= 210
    elif where == "q":
        a[6][7, 0] = 1 << 29
    else:
        a[5][0, 0] = -1
    rng = np.random.RandomState(2)
    prev = (rng.normal(size=(N_VARS, N_VARS)).astype(F),
            rng.normal(size=N_VARS).astype(F), np.array([1.0], F))
    st, A, b, res = run_alignment_seam(a, 0.05, prev=prev)
    assert st == INVALID_ARG
    for got, was in zip((A, b, res), prev):
        assert got.tobytes() == was.tobytes()


# ---- regularizer seam --------------------------------------------------------

def run_regularizer_seam(g, curr, masks, weight, anchor):
    from open3d_amd import slac
    AtA = torch.zeros((N_VARS, N_VARS), dtype=torch.float32, device="cuda")
    Atb = torch.zeros(N_VARS, dtype=torch.float32, device="cuda")
    res = torch.zeros(1, dtype=torch.float32, device="cuda")
    st = slac.fill_in_slac_regularizer_term_raw(
        AtA, Atb, res, _cuda(np.arange(len(g.keys), dtype=np.int32)),
        _cuda(g.nbs_idx.astype(np.int32)), _cuda(masks), _cuda(g.init),
        _cuda(curr), weight, N_FRAGS, anchor)
    return st, AtA.cpu().numpy(), Atb.cpu().numpy(), res.cpu().numpy()


def regularizer_deviation(name, g, curr, masks):
    want = no.regularizer(np.arange(64), g.nbs_idx, masks, g.init, curr,
                          F(3.0), N_FRAGS, g.anchor, N_VARS)
    st, A, b, res = run_regularizer_seam(g, curr, masks, 3.0, g.anchor)
    assert st == 0
    dev = max(np.abs(A - want["AtA"]).max() / np.abs(want["AtA"]).max(),
              np.abs(b - want["Atb"]).max() /
              max(np.abs(want["Atb"]).max(), 1.0),
              abs(res[0] - want["residual"]) / max(want["residual"], 1.0))
    return float(dev), want, (A, b, res)


@pytest.mark.parametrize("case", range(4))
def test_regularizer_seam_matches_the_oracle(case):
    name, g, curr, masks = regularizer_cases()[case]
    dev, want, (A, b, res) = regularizer_deviation(name, g, curr, masks)
    print("regularizer %s: max relative deviation %.3g" % (name, dev))
    assert dev <= 16 * REG_DEVIATION
    assert np.array_equal(A, A.T)
    assert not A[:18].any() and not b[:18].any()
    if name == "identity":
        assert not b.any() and res[0] == 0
    if name == "starved":
        assert 21 not in want["sigma"]
    if name == "mirrored":
        assert res[0] > 1.0     # a reflection is not a rotation


def test_regularizer_seam_rejects_a_node_outside_the_system():
    name, g, curr, masks = regularizer_cases()[1]
    from open3d_amd import slac
    AtA = torch.ones((N_VARS, N_VARS), dtype=torch.float32, device="cuda")
    Atb = torch.ones(N_VARS, dtype=torch.float32, device="cuda")
    res = torch.ones(1, dtype=torch.float32, device="cuda")
    nb = g.nbs_idx.astype(np.int32)
    nb[5, np.nonzero(masks[5])[0][0]] = 64
    st = slac.fill_in_slac_regularizer_term_raw(
        AtA, Atb, res, _cuda(np.arange(64, dtype=np.int32)), _cuda(nb),
        _cuda(masks), _cuda(np.concatenate([g.init, g.init])),
        _cuda(np.concatenate([curr, curr])), 3.0, N_FRAGS, g.anchor)
    assert st == INVALID_ARG
    assert bool((AtA == 1).all()) and bool((Atb == 1).all()) and \
        float(res[0]) == 1.0


# ---- solver ----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, PANEL - 1, PANEL, PANEL + 1, 2 * PANEL + 3,
                               210])
def test_solve_spd_is_backward_stable(n):
    from open3d_amd import slac
    rng = np.random.RandomState(n)
    B = rng.normal(size=(n, n)) / np.sqrt(n)
    A = B.T @ B + np.eye(n)
    assert np.linalg.cond(A) < 1e6
    b = rng.normal(size=n)
    low = np.tril(A) + np.triu(np.full((n, n), np.nan), 1)
    x = slac.solve_spd(_cuda(low), _cuda(b)).cpu().numpy()
    assert np.all(np.isfinite(x))
    resid = np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) *
                                         np.linalg.norm(x) +
                                         np.linalg.norm(b))
    ref = np.linalg.solve(A, b)
    print("n %d: relative residual %.3g (bound %.3g), |x - ref| %.3g" %
          (n, resid, 64 * n * 2.0 ** -53, np.abs(x - ref).max()))
    assert resid <= 64 * n * 2.0 ** -53


def test_solve_spd_reports_a_zero_pivot_and_too_many_unknowns():
    from open3d_amd import slac
    A = np.eye(70)
    A[40, 40] = 0.0
    assert slac.solve_spd_raw(_cuda(A), _cuda(np.ones(70))) == SINGULAR
    A[40, 40] = np.nan
    assert slac.solve_spd_raw(_cuda(A), _cuda(np.ones(70))) == SINGULAR
    tiny = torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    big = torch.zeros(32769, dtype=torch.float64, device="cuda")
    # n is checked before anything is allocated or launched: a {1,1} matrix
    # stands in for the 8.6 GB one
    assert slac.solve_spd_raw(tiny, big) == UNSUPPORTED


# ---- driver ----------------------------------------------------------------

def gpu_run(iterations, grid=None, poses=None, fragments=None, edges=None):
    from open3d_amd import slac
    frags, start, ed, _ = scene()
    frags = fragments if fragments is not None else frags
    ed = edges if edges is not None else ed
    fc = [(_cuda(p), _cuda(n)) for p, n in frags]
    params = slac.SLACOptimizerParams(max_iterations=iterations)
    grid = grid if grid is not None else slac.ControlGrid(GRID_SIZE, 1000)
    st, P, info = slac.slac_optimize_raw(
        fc, poses if poses is not None else start, ed, params, grid)
    return st, P, info, grid


def nodes_by_key(grid):
    """{key: current position} of a device grid."""
    active, _, _ = grid.get_neighbor_grid_map()
    a = active.long()
    curr = grid.get_curr_positions()[a].cpu().numpy()
    init = grid.get_init_positions()[a].cpu().numpy()
    keys = np.rint(init / F(grid.grid_size)).astype(np.int32)
    return {tuple(int(v) for v in k): c for k, c in zip(keys, curr)}


def test_optimizer_follows_the_oracle():
    from open3d_amd import slac
    frags, start, edges, ogrid = scene()
    want = oracle_run(3, pin_anchor=True)
    assert want["status"] == "ok" and want["skipped"] == 0
    st, P, info, grid = gpu_run(3)
    assert st == 0
    assert info["kept"] == want["kept"] and \
        info["n_corres"] == want["n_corres"] and info["skipped"] == 0
    assert grid.size() == len(ogrid.keys)
    got_nodes = nodes_by_key(grid)
    curr = np.array([got_nodes[tuple(int(v) for v in k)] for k in ogrid.keys],
                    F)
    assert np.array_equal(curr[ogrid.anchor], ogrid.init[ogrid.anchor])
    node_dev = float(np.abs(curr - want["curr"]).max())
    pose_dev = float(np.abs(P - np.stack(want["poses"])).max())
    loss_dev = np.abs(info["alignment_losses"] -
                      np.array(want["alignment_losses"])) / \
        np.array(want["alignment_losses"])
    reg_dev = np.abs(info["regularizer_losses"] -
                     np.array(want["regularizer_losses"]))
    print("driver: pose deviation %.3g, node deviation %.3g, loss deviations "
          "%s, regularizer loss deviations %s" %
          (pose_dev, node_dev, loss_dev.tolist(), reg_dev.tolist()))
    print("losses", info["alignment_losses"].tolist(),
          info["regularizer_losses"].tolist())
    assert pose_dev <= 16 * DRIVER_POSE_DEVIATION
    assert node_dev <= NODE_BOUND
    assert np.all(loss_dev <= np.array(LOSS_BOUNDS))
    # lower than where it started and than the rigid optimizer gets
    fc = [(_cuda(p), _cuda(n)) for p, n in frags]
    _, rinfo = slac.run_rigid_optimizer_for_fragments(
        fc, slac.PoseGraph(start, edges),
        slac.SLACOptimizerParams(max_iterations=3), return_info=True)
    al = info["alignment_losses"]
    assert al[-1] < al[0] and al[-1] < rinfo["losses"][-1]
    # the returned grid and poses bring the kept correspondences together
    sets = [so.correspondence_set(frags[i][0], frags[j][0], i, j, start[i],
                                  start[j], T, 0.07, 0.3)["corres"]
            for i, j, T in edges]
    dgrid = no.Grid(ogrid.keys, GRID_SIZE, curr)
    before = no.mean_plane_residual(frags, start, edges, sets)
    after = no.mean_plane_residual(frags, list(P), edges, sets, dgrid)
    print("mean point-to-plane residual %.4g -> %.4g" % (before, after))
    assert after < before


def test_optimizer_continues_from_a_returned_grid():
    st3, P3, _, grid = gpu_run(3)
    assert st3 == 0
    st1, P31, info1, grid = gpu_run(1, grid=grid, poses=list(P3))
    st4, P4, info4, grid4 = gpu_run(4)
    assert st1 == 0 and st4 == 0
    # the correspondence sets depend on T_ij and the fragments only (the
    # poses enter the kept / dropped decision alone), so the continued run
    # has the sets of the four-iteration run and the same state goes into the
    # fourth iteration. The grid entries are atomic sums, so x agrees to
    # rounding: a node may land on the next float32 (2^-22 below 2 m, twice
    # for safety), a pose entry moves by that times the step's sensitivity,
    # far below 1e-9
    assert info1["kept"] == info4["kept"]
    assert info1["n_corres"] == info4["n_corres"]
    a, b = nodes_by_key(grid), nodes_by_key(grid4)
    assert a.keys() == b.keys()
    assert np.abs(P31 - P4).max() <= 1e-9
    assert max(float(np.abs(a[k] - b[k]).max()) for k in a) <= 2.0 ** -21
    assert abs(info1["alignment_losses"][0] - info4["alignment_losses"][3]) \
        <= 1e-9 * info4["alignment_losses"][3]


def test_optimizer_counts_pairs_in_cells_with_an_inactive_corner():
    from open3d_amd import slac
    frags, start, edges, ogrid = scene()
    drop = len(ogrid.keys) // 3
    keys = np.delete(ogrid.keys, drop, axis=0)
    small = no.Grid(keys, GRID_SIZE)
    want = no.slac_optimize(frags, start, edges, small, 1)
    assert want["skipped"] > 0
    grid = slac.ControlGrid(GRID_SIZE, keys=_cuda(keys), values=_cuda(small.init))
    grid.compactify()
    st, P, info, _ = gpu_run(1, grid=grid)
    assert st == 0 and info["skipped"] == want["skipped"]
    assert info["n_inliers"] == want["n_inliers"]


def test_optimizer_error_paths_leave_poses_and_grid_alone():
    from open3d_amd import slac
    frags, start, edges, ogrid = scene()
    st, P, _, _ = gpu_run(2, edges=[(0, 3, np.eye(4))])
    assert st == INVALID_ARG and np.array_equal(P, np.stack(start))
    empty = [frags[0], (np.zeros((0, 3), F), np.zeros((0, 3), F)), frags[2]]
    st, P, _, _ = gpu_run(2, fragments=empty)
    assert st == INVALID_ARG and np.array_equal(P, np.stack(start))
    # no edges: fragments 1 and 2 have no equation
    grid = slac.ControlGrid(GRID_SIZE, 1000)
    grid.touch(_cuda(frags[0][0]))
    grid.compactify()
    curr = grid.get_curr_positions().clone()
    st, P, _, grid = gpu_run(2, grid=grid, edges=[])
    assert st == SINGULAR and np.array_equal(P, np.stack(start))
    assert torch.equal(grid.get_curr_positions(), curr)
