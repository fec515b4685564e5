"""Rigid multiway fragment optimisation on the MI355X against the numpy
restatement (tests/_slac_oracle.py): the batched terms kernel, the reference's
seam form, the correspondence set of an edge and the whole optimizer."""
import functools

import numpy as np
import pytest
import torch

import _slac_oracle as so

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, SINGULAR, UNSUPPORTED = 1, 5, 7
COUNTS = [0, 1, 63, 64, 65, 100003]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frags_cuda(frags):
    return [(_cuda(p), _cuda(n)) for p, n in frags]


@functools.lru_cache(maxsize=None)
def _terms_world():
    """4 fragments: the same 30 k surface points, each with its own noise, its
    own row order and its own small pose error, so that matched rows are a few
    centimetres apart and a 2 cm threshold splits them."""
    rng = np.random.RandomState(21)
    base, nrm = so.surface(30000, 4)
    frags, inv, poses = [], [], []
    for k in range(4):
        perm = rng.permutation(base.shape[0])
        p = base + rng.normal(0, 0.01, base.shape)
        frags.append((p[perm].astype(F), nrm[perm].astype(F)))
        iv = np.empty_like(perm)
        iv[perm] = np.arange(perm.size)
        inv.append(iv)
        poses.append(so._rigid(rng, 0.5, 0.01))
    return frags, inv, poses


def _pairs(inv, i, j, count, seed):
    m = np.random.RandomState(seed).randint(0, inv[i].size, count)
    return np.stack([inv[i][m], inv[j][m]], 1).astype(np.int64).reshape(-1, 2)


def _check_terms(edges, counts, threshold=0.02):
    from open3d_amd import slac
    frags, inv, poses = _terms_world()
    sets = [_pairs(inv, i, j, c, 100 + e)
            for e, ((i, j), c) in enumerate(zip(edges, counts))]
    got = slac.rigid_terms(_frags_cuda(frags), poses, edges,
                           [_cuda(c) for c in sets], threshold)
    again = slac.rigid_terms(_frags_cuda(frags), poses, edges,
                             [_cuda(c) for c in sets], threshold)
    assert torch.equal(got, again), "two runs differ"
    got = got.cpu().numpy()
    for e, (i, j) in enumerate(edges):
        want, mag = so.edge_sums(frags[i], frags[j], sets[e], poses[i],
                                 poses[j], threshold)
        assert got[e, 28] == want[28], (e, got[e, 28], want[28])
        if counts[e] > 1000:
            assert 0 < want[28] < counts[e]  # both sides of the threshold
        err = np.abs(got[e, :28] - want[:28])
        print("edge %d count %d: worst |err| / sum|terms| = %.3g" %
              (e, counts[e], float((err / np.maximum(mag, 1e-300)).max())))
        # identical float32 terms, another float64 order:
        # n * eps(float64) * sum |x|, n <= 1e5, rounded up
        assert np.all(err <= 1e-12 * mag), (e, err, mag)
        if counts[e] == 0:
            assert not got[e].any()


@pytest.mark.parametrize("count", COUNTS)
def test_rigid_terms_one_edge(count):
    _check_terms([(1, 3)], [count])


def test_rigid_terms_seven_edges():
    edges = [(0, 1), (1, 2), (2, 3), (0, 2), (3, 1), (0, 3), (2, 0)]
    _check_terms(edges, [100003] + COUNTS)


def test_rigid_terms_all_pairs_beyond_threshold_give_zeros():
    from open3d_amd import slac
    frags, inv, poses = _terms_world()
    cs = _pairs(inv, 0, 1, 5000, 7)
    want, _ = so.edge_sums(frags[0], frags[1], cs, poses[0], poses[1], 1e-9)
    assert want[28] == 0
    got = slac.rigid_terms(_frags_cuda(frags), poses, [(0, 1)], [_cuda(cs)],
                           1e-9)
    assert not got.cpu().numpy().any()


def test_rigid_terms_keep_r_equal_to_threshold():
    """|r| == threshold is kept (the reference skips on >). Identity poses
    leave the coordinates as they are, so r is 0.25 exactly in rows 0, 1."""
    from open3d_amd import slac
    pi = np.array([[0.5, 0, 0], [0.5, 1, 0], [0.5, 2, 0]], F)
    ni = np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0]], F)
    pj = np.array([[0.25, 0, 0], [0.25, 1, 0], [0.125, 2, 0]], F)
    nj = np.zeros((3, 3), F)
    cs = np.array([[0, 0], [1, 1], [2, 2]], np.int64)
    I = np.eye(4)
    want, _ = so.edge_sums((pi, ni), (pj, nj), cs, I, I, 0.25)
    assert want[28] == 2
    got = slac.rigid_terms(_frags_cuda([(pi, ni), (pj, nj)]), [I, I],
                           [(0, 1)], [_cuda(cs)], 0.25).cpu().numpy()
    assert got[0, 28] == 2
    assert np.array_equal(got[0], want)  # two terms: every order is the same


def test_rigid_terms_out_of_range_index_is_refused():
    from open3d_amd import _lib, slac
    frags, inv, poses = _terms_world()
    n1 = frags[1][0].shape[0]
    for bad_row in ([5, n1], [-1, 3], [frags[0][0].shape[0], 0]):
        cs = _pairs(inv, 0, 1, 3000, 9)
        cs[1234] = bad_row
        out = torch.full((1, 29), -7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.O3DMIError) as e:
            slac.rigid_terms(_frags_cuda(frags), poses, [(0, 1)], [_cuda(cs)],
                             0.02, out=out)
        assert e.value.status == INVALID_ARG
        assert bool((out == -7.0).all()), "the output was written"


def test_seam_form_scatters_one_edge_into_a_four_node_system():
    from open3d_amd import slac
    frags, inv, poses = _terms_world()
    cs = _pairs(inv, 1, 3, 5000, 13)
    p = so.transform_rows(poses[1], frags[1][0][cs[:, 0]])
    n = so.rotate_rows(poses[1], frags[1][1][cs[:, 0]])
    q = so.transform_rows(poses[3], frags[3][0][cs[:, 1]])
    take, terms, _, _ = so.pair_terms(p, q, n, 0.02)
    sums, _ = so.sum_terms(take, terms)
    rng = np.random.RandomState(3)
    AtA = rng.uniform(-50, 50, (24, 24)).astype(F)   # the sentinel prefill
    Atb = rng.uniform(-50, 50, 24).astype(F)
    res = np.array([3.25], F)
    for (i, j) in ((1, 3), (3, 1)):
        wA, wb, wr = so.scatter_seam(AtA, Atb, res, sums, i, j)
        gA, gb, gr = _cuda(AtA), _cuda(Atb), _cuda(res)
        slac.fill_in_rigid_alignment_term(gA, gb, gr, _cuda(p), _cuda(q),
                                          _cuda(n), i, j, 0.02)
        gA, gb, gr = gA.cpu().numpy(), gb.cpu().numpy(), gr.cpu().numpy()
        assert np.array_equal(gA, wA)
        assert np.array_equal(gb, wb)
        assert np.array_equal(gr, wr)
        rows = [6 * i + k for k in range(6)] + [6 * j + k for k in range(6)]
        outside = np.ones((24, 24), bool)
        outside[np.ix_(rows, rows)] = False
        assert np.array_equal(gA[outside], AtA[outside])
        assert not np.array_equal(gA[~outside], AtA[~outside])
        other = np.setdiff1d(np.arange(24), rows)
        assert np.array_equal(gb[other], Atb[other])


def test_seam_form_refuses_bad_node_ids():
    from open3d_amd import _lib, slac
    z = torch.zeros((8, 3), device="cuda")
    for (i, j) in ((1, 1), (0, 4), (-1, 2)):
        A = torch.zeros((24, 24), device="cuda")
        with pytest.raises(_lib.O3DMIError) as e:
            slac.fill_in_rigid_alignment_term(
                A, torch.zeros(24, device="cuda"),
                torch.zeros(1, device="cuda"), z, z, z, i, j, 0.07)
        assert e.value.status == INVALID_ARG


@functools.lru_cache(maxsize=None)
def _scene():
    frags, truth, start, edges = so.make_scene()
    return frags, truth, start, edges


def test_correspondence_set_equals_the_oracle_row_for_row():
    from open3d_amd import slac
    frags, _, start, edges = _scene()
    g = _frags_cuda(frags)
    for (i, j, T_ij) in (edges[0], edges[4]):
        want = so.correspondence_set(frags[i][0], frags[j][0], i, j, start[i],
                                     start[j], T_ij, 0.07, 0.3)
        got, info = slac.get_correspondence_set_for_point_cloud_pair(
            i, j, g[i][0], g[j][0], start[i], start[j], T_ij, 0.07, 0.3,
            return_info=True)
        assert want["kept"] and info["kept"]
        assert want["corres"].shape[0] >= 1000
        assert np.array_equal(got.cpu().numpy(), want["corres"])
        assert info["n_inliers"] == want["inliers"]
        assert 0 < want["inliers"] < want["corres"].shape[0]
        assert info["inlier_ratio"] == want["ratio"]


def test_correspondence_set_pruning_branches():
    from open3d_amd import slac
    rng = np.random.RandomState(5)
    a = rng.uniform(-1, 1, (500, 3)).astype(F)
    ga = _cuda(a)
    I = np.eye(4)
    far = np.eye(4)
    far[0, 3] = 5.0

    def run(i, j, T_i, T_j, T_ij):
        want = so.correspondence_set(a, a, i, j, T_i, T_j, T_ij, 0.07, 0.3)
        got, info = slac.get_correspondence_set_for_point_cloud_pair(
            i, j, ga, ga, T_i, T_j, T_ij, 0.07, 0.3, return_info=True)
        assert info["kept"] == want["kept"]
        assert info["n_corres"] == want["corres"].shape[0]
        assert info["n_inliers"] == want["inliers"]
        assert np.array_equal(info["all_pairs"].cpu().numpy(), want["corres"])
        assert got.shape[0] == (info["n_corres"] if info["kept"] else 0)
        return info

    odo = run(3, 4, I, far, I)
    assert odo["kept"] and odo["inlier_ratio"] == 0     # j == i + 1
    assert not run(3, 5, I, far, I)["kept"]             # ratio 0 < 0.3
    assert run(3, 5, I, I, I)["kept"]
    none = run(3, 4, I, I, far)                         # C == 0
    assert not none["kept"] and none["n_corres"] == 0
    assert np.isnan(none["inlier_ratio"])


def test_correspondence_set_inlier_test_is_less_or_equal():
    from open3d_amd import slac
    d = F(0.25)
    p = np.zeros((2, 3), F)
    p[1, 1] = 10.0
    q = np.array([[0.25, 0, 0], [np.nextafter(F(0.25), F(1)), 10, 0]], F)
    T_ij = np.eye(4)
    T_ij[0, 3] = 0.25
    _, info = slac.get_correspondence_set_for_point_cloud_pair(
        0, 1, _cuda(p), _cuda(q), np.eye(4), np.eye(4), T_ij, d, 0.3,
        return_info=True)
    assert info["n_corres"] == 2 and info["n_inliers"] == 1
    assert info["inlier_ratio"] == F(0.5)


def test_whole_optimizer_on_the_scene():
    """Against the restatement at upstream's defaults (5 iterations, 0.07,
    0.3). The pose tolerance is measured on the oracle alone: d = the largest
    pose-entry difference between two oracle runs whose float64 sums run in
    opposite orders (measured: d = 2.8e-16); allowed 10 d, at least 1e-12 (the
    GPU's tree is a third order). Losses: the sums' relative 1e-12."""
    from open3d_amd import slac
    frags, truth, start, edges = _scene()
    want = so.rigid_optimize(frags, start, edges)
    rev = so.rigid_optimize(frags, start, edges, reverse=True)
    d = max(float(np.abs(a - b).max())
            for a, b in zip(want["poses"], rev["poses"]))
    tol = max(10 * d, 1e-12)
    graph = slac.PoseGraph(start, edges)
    got, info = slac.run_rigid_optimizer_for_fragments(
        _frags_cuda(frags), graph, slac.SLACOptimizerParams(),
        return_info=True)
    assert info["kept"] == want["kept"] == [True] * len(edges)
    assert info["n_corres"] == want["n_corres"]
    assert info["n_inliers"] == want["n_inliers"]
    worst = max(float(np.abs(a - b).max())
                for a, b in zip(got.nodes, want["poses"]))
    print("oracle order sensitivity d = %.3g, tolerance %.3g, worst pose "
          "entry difference %.3g" % (d, tol, worst))
    assert worst <= tol, (worst, tol)
    gl, wl = info["losses"], np.array(want["losses"])
    print("losses", gl, wl)
    assert gl.shape == wl.shape == (5,)
    assert np.all(np.abs(gl - wl) <= 1e-12 * wl)
    before = so.relative_errors(start, truth)
    after = so.relative_errors(got.nodes, truth)
    for b, a in zip(before, after):
        assert a[0] <= b[0] / 2 and a[1] <= b[1] / 2


def test_whole_optimizer_error_paths():
    from open3d_amd import _lib, slac
    frags, _, start, edges = _scene()
    g = _frags_cuda(frags)
    params = slac.SLACOptimizerParams()

    st, _, _ = slac.rigid_optimize_raw([g[0]] * 513, [np.eye(4)] * 513,
                                       [(0, 1, np.eye(4))], params)
    assert st == UNSUPPORTED
    st, _, _ = slac.rigid_optimize_raw(g, start, [(2, 2, np.eye(4))], params)
    assert st == INVALID_ARG
    st, _, _ = slac.rigid_optimize_raw(g, start, [(0, 5, np.eye(4))], params)
    assert st == INVALID_ARG

    # node 4 is reached by no edge: its six rows are zero
    st, P, _ = slac.rigid_optimize_raw(g, start, edges[:3], params)
    assert st == SINGULAR
    assert np.array_equal(P, np.stack(start))
    with pytest.raises(_lib.O3DMIError):
        slac.run_rigid_optimizer_for_fragments(
            g, slac.PoseGraph(start, edges[:3]), params)

    want = so.rigid_optimize(frags, start, edges, max_iterations=0)
    st, P, info = slac.rigid_optimize_raw(
        g, start, edges, slac.SLACOptimizerParams(max_iterations=0))
    assert st == 0 and np.array_equal(P, np.stack(start))
    assert info["kept"] == want["kept"]
    assert info["n_corres"] == want["n_corres"]
    assert info["losses"].size == 0
