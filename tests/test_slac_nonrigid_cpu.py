"""CPU self-checks of the non-rigid SLAC oracle (tests/_slac_nonrigid_oracle.py)
and of the inputs the GPU tests rely on."""
import numpy as np

import _slac_nonrigid_oracle as no
import _slac_oracle as so

F = np.float32


def test_block_equals_the_reference_double_loop():
    arrays = no.seam_inputs(50, 77)
    take, J, idx, r = no.pair_jacobians(*arrays, 1, 2, no.N_FRAGS, 0.05)
    assert 0 < take.sum() < 50
    A, b, res = no.upstream_double_loop(J[take], idx[take], r[take], no.N_VARS)
    A2, b2, res2 = no.naive_system(take, J, idx, r, no.N_VARS)
    assert np.array_equal(A, A2) and np.array_equal(b, b2) and res == res2
    want = no.exact_system(take, J, idx, r, no.N_VARS)
    assert np.allclose(A, want["AtA"], rtol=0, atol=50 * 2.0 ** -52 *
                       want["mag_A"].max())
    assert np.array_equal(want["AtA"], want["AtA"].T)
    # the 60 indices: 6 i.., 6 j.., then 3 per corner behind 6 n_frags
    assert idx[0, :12].tolist() == list(range(6, 18))
    assert idx[0, 12] == 18 + 3 * arrays[5][0, 0] and \
        idx[0, 59] == 18 + 3 * arrays[6][0, 7] + 2


def test_dyadic_case_sums_exactly_in_both_orders():
    arrays = no.seam_inputs(1500, 5, dyadic=True)
    take, J, idx, r = no.pair_jacobians(*arrays, 1, 2, no.N_FRAGS, 0.0625)
    assert 0 < take.sum() < 1500
    want = no.exact_system(take, J, idx, r, no.N_VARS)
    for reverse in (False, True):
        A, b, res = no.naive_system(take, J, idx, r, no.N_VARS, reverse)
        assert np.array_equal(A, want["AtA"]) and \
            np.array_equal(b, want["Atb"]) and res == want["residual"]


def test_regularizer_of_an_undeformed_grid_is_at_rest():
    name, g, curr, masks = no.regularizer_cases()[0]
    out = no.regularizer(np.arange(64), g.nbs_idx, masks, g.init, curr, F(3),
                         3, g.anchor, no.N_VARS)
    assert not out["Atb"].any() and out["residual"] == 0
    assert np.array_equal(out["AtA"], out["AtA"].T)


def test_regularizer_of_a_rigidly_rotated_grid_has_no_residual():
    name, g, curr, masks = no.regularizer_cases()[0]
    R = so._rigid(np.random.RandomState(3), 25.0, 0.2)
    rot = (g.init.astype(np.float64) @ R[:3, :3].T + R[:3, 3]).astype(F)
    out = no.regularizer(np.arange(64), g.nbs_idx, masks, g.init, rot, F(3),
                         3, -1, no.N_VARS)
    # float32 positions: each local residual is a few float32 roundings of
    # coordinates below 4
    assert out["residual"] <= 3 * 64 * 6 * 3 * (8 * 2.0 ** -22) ** 2
    # at the anchor the identity replaces the rotation
    out = no.regularizer(np.arange(64), g.nbs_idx, masks, g.init, rot, F(3),
                         3, g.anchor, no.N_VARS)
    assert out["residual"] > 1e-3


def test_regularizer_inputs_keep_the_second_singular_value_up():
    for name, g, curr, masks in no.regularizer_cases():
        out = no.regularizer(np.arange(64), g.nbs_idx, masks, g.init, curr,
                             F(3), 3, g.anchor, no.N_VARS)
        for S in out["sigma"].values():
            assert S[1] > 0.1 * S[0], (name, S)
    assert np.linalg.det(no.local_rotation(-np.eye(3))[0]) > 0


def test_oracle_driver_beats_the_rigid_optimizer_on_the_scene():
    want = no.oracle_run(3)
    frags, start, edges, grid = no.scene()
    assert want["status"] == "ok" and all(want["kept"])
    rigid = so.rigid_optimize(frags, start, edges, 3)
    al = want["alignment_losses"]
    assert al[-1] < al[0] and al[-1] < rigid["losses"][-1]
    assert 2500 < frags[0][0].shape[0] < 4500


def test_lu_and_pinned_oracle_differ_by_the_gauge_only():
    """The reference's system is singular: its LU moves the anchor node by
    centimetres, the pinned solve not at all, and after three iterations both
    agree in what every solution shares."""
    lu, pin = no.oracle_run(3), no.oracle_run(3, pin_anchor=True)
    frags, start, edges, grid = no.scene()
    a = grid.anchor
    assert np.array_equal(pin["curr"][a], grid.init[a])
    assert np.abs(lu["curr"][a] - grid.init[a]).max() > 1e-3
    rel = (lu["curr"] - lu["curr"][a]) - (pin["curr"] - pin["curr"][a])
    # float32 nodes around 2 m carry 2^-22; three iterations of a solve
    # whose first LU step is off by 1e-3 m leave a few of those
    assert np.abs(rel).max() < 1e-4
    assert abs(lu["alignment_losses"][2] - pin["alignment_losses"][2]) < \
        1e-3 * pin["alignment_losses"][2]
    al = pin["alignment_losses"]
    rigid = so.rigid_optimize(frags, start, edges, 3)
    assert al[-1] < al[0] and al[-1] < rigid["losses"][-1]
