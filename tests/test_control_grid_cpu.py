"""Self-checks of the ControlGrid oracle (tests/_control_grid_oracle.py): the
properties of the trilinear embedding the GPU tests rely on."""
import numpy as np

import _control_grid_oracle as co

F = np.float32
EPS = float(np.finfo(F).eps)
GRID = 0.375


def _cloud(n=2000, seed=3):
    rng = np.random.RandomState(seed)
    p = rng.uniform(-0.75, 0.75, (n, 3)).astype(F)
    # some points exactly on lattice planes (0.375 k is exact in float32)
    p[:60, 0] = (rng.randint(-2, 2, 60) * GRID).astype(F)
    p[30:90, 2] = (rng.randint(-2, 2, 60) * GRID).astype(F)
    nm = rng.normal(size=(n, 3))
    nm /= np.linalg.norm(nm, axis=1, keepdims=True)
    return p, nm.astype(F)


def _embedded(p, nm):
    keys, _ = co.touch(p, GRID)
    return keys, co.parameterize(p, GRID, co.key_set(keys), nm)


def test_vertex_ratios_are_a_partition_of_unity():
    p, nm = _cloud()
    _, par = _embedded(p, nm)
    assert par["valid"].all()
    assert (par["vertex"] >= 0).all()
    err = np.abs(par["vertex"].astype(np.float64).sum(1) - 1.0)
    print("worst |sum - 1| = %.3g (%.2f ulp)" % (err.max(), err.max() / EPS))
    assert err.max() <= 4 * EPS


def test_normal_ratios_sum_to_zero():
    p, nm = _cloud()
    _, par = _embedded(p, nm)
    err = np.abs(par["normal"].astype(np.float64).sum(1))
    print("worst |sum| = %.3g (%.2f ulp)" % (err.max(), err.max() / EPS))
    assert err.max() <= 4 * EPS


def test_deform_through_untouched_grid_is_identity():
    p, nm = _cloud()
    keys, par = _embedded(p, nm)
    grid = co.identity_grid(keys, GRID)
    pos, nrm = co.deform(co.corner_positions(par["keys"], grid),
                         par["vertex"], par["normal"])
    err = np.abs(pos.astype(np.float64) - p).max()
    print("worst |deform(p) - p| = %.3g" % err)
    assert err <= 4 * EPS * np.abs(p).max()
    # the embedded normal comes back as a unit vector along the input
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() \
        < 1e-5
    assert (np.sum(nrm * nm, 1) > 0.999).all()


def test_point_on_a_lattice_plane():
    p = np.array([[0.375, -0.75, 0.1], [-0.375, 0.2, 0.75]], F)
    fl, res, ok = co.quantize(p, GRID)
    assert ok.all()
    assert fl[0, 0] == 1 and fl[0, 1] == -2 and fl[1, 0] == -1 \
        and fl[1, 2] == 2
    assert res[0, 0] == 0 and res[0, 1] == 0 and res[1, 2] == 0
    keys, _ = co.touch(p, GRID)
    par = co.parameterize(p, GRID, co.key_set(keys))
    # ratio 0 on every corner of the far side of the plane the point lies on
    far_x = co.CORNERS[:, 0] == 1
    assert (par["vertex"][0, far_x] == 0).all()
    assert (par["vertex"][0, ~far_x].sum() == 1)
    far_z = co.CORNERS[:, 2] == 1
    assert (par["vertex"][1, far_z] == 0).all()


def test_non_finite_and_out_of_range_points_are_never_valid():
    p = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
                  [1e9, 0, 0], [0.1, 0.1, 0.1]], F)
    _, _, ok = co.quantize(p, GRID)
    assert ok.tolist() == [False, False, False, False, True]
    keys, vals = co.touch(p, GRID)
    assert len(keys) == 8
    assert np.array_equal(vals, keys.astype(F) * F(GRID))


def test_anchor_is_the_zyx_median():
    rng = np.random.RandomState(5)
    keys = np.unique(rng.randint(-4, 5, (200, 3)).astype(np.int32), axis=0)
    rng.shuffle(keys)
    want = sorted((int(z), int(y), int(x)) for x, y, z in keys)[len(keys) // 2]
    assert co.anchor_key(keys) == (want[2], want[1], want[0])


def test_projection_takes_the_smallest_depth_then_the_lowest_index():
    K = np.array([[50.0, 0, 4.0], [0, 50.0, 3.0], [0, 0, 1]])
    T = np.eye(4)
    pts = np.array([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0], [9, 0, 1.0],
                    [0, 0, -1.0], [0, 0, 5.0]], F)
    cols = np.arange(18, dtype=F).reshape(6, 3)
    depth, color, hits = co.project(pts, K, T, 6, 8, 1000.0, 3.0, cols,
                                    return_hits=True)
    assert hits[3 * 8 + 4] == 3 and hits.sum() == 3
    assert depth[3, 4] == 1000.0 and np.count_nonzero(depth) == 1
    assert np.array_equal(color[3, 4], cols[1])


def test_new_entry_points_are_declared_and_bound():
    import os

    from open3d_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_h = open(os.path.join(root, "include", "o3d_mi355x_host.h")).read()
    names = [n for n in _lib.PROTOTYPES
             if n.startswith("o3dmi_control_grid_") or
             n.startswith("o3dmi_project_to_")]
    assert len(names) == 18
    for name in names:
        assert name + "(" in host_h, name
