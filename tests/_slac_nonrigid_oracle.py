"""numpy restatement of the non-rigid half of t::pipelines::slac:

    FillInSLACAlignmentTerm{CPU,CUDA}    kernel/FillInLinearSystemImpl.h:156-312
    FillInSLACRegularizerTerm{CPU,CUDA}  kernel/FillInLinearSystemImpl.h:314-524
    FillInSLACAlignmentTerm (per edge)   slac/FillInLinearSystemImpl.h:102-150
    RunSLACOptimizerForFragments         slac/SLACOptimizer.cpp:253-367

Per-pair terms are np.float32 in the reference's expression order; sums are
float64 (exactly rounded with math.fsum where a test needs the order-free
value), the regularizer's rotation comes from numpy.linalg.svd in float64 and
the solve is numpy.linalg.solve in float64.
"""
import functools
import math

import numpy as np

import _control_grid_oracle as cg
import _oracle as orc
import _slac_oracle as so

F = np.float32


def pair_jacobians(Ti_Cps, Tj_Cqs, Cnormal_ps, Ri_Cnormal_ps,
                   RjT_Ri_Cnormal_ps, idx_ps, idx_qs, ratio_ps, ratio_qs, i, j,
                   n_frags, threshold):
    """-> (take {m} bool, J {m,60} float32, idx {m,60} int64, r {m} float32):
    the reference's J and idx of every pair."""
    p, q, cn, n, v = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in
                      (Ti_Cps, Tj_Cqs, Cnormal_ps, Ri_Cnormal_ps,
                       RjT_Ri_Cnormal_ps))
    ip = np.asarray(idx_ps, np.int64).reshape(-1, 8)
    iq = np.asarray(idx_qs, np.int64).reshape(-1, 8)
    rp = np.ascontiguousarray(ratio_ps, F).reshape(-1, 8)
    rq = np.ascontiguousarray(ratio_qs, F).reshape(-1, 8)
    m = p.shape[0]
    r = (p[:, 0] - q[:, 0]) * n[:, 0] + (p[:, 1] - q[:, 1]) * n[:, 1]
    r = r + (p[:, 2] - q[:, 2]) * n[:, 2]
    take = ~(np.abs(r) > F(threshold))
    J = np.zeros((m, 60), F)
    idx = np.zeros((m, 60), np.int64)
    J[:, 0] = -q[:, 2] * n[:, 1] + q[:, 1] * n[:, 2]
    J[:, 1] = q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2]
    J[:, 2] = -q[:, 1] * n[:, 0] + q[:, 0] * n[:, 1]
    J[:, 3:6] = n
    J[:, 6:12] = -J[:, 0:6]
    for k in range(6):
        idx[:, k] = 6 * i + k
        idx[:, 6 + k] = 6 * j + k
    for k in range(8):
        for a in range(3):
            J[:, 12 + 3 * k + a] = rp[:, k] * cn[:, a]
            idx[:, 12 + 3 * k + a] = 6 * n_frags + 3 * ip[:, k] + a
            J[:, 36 + 3 * k + a] = (-rq[:, k]) * v[:, a]
            idx[:, 36 + 3 * k + a] = 6 * n_frags + 3 * iq[:, k] + a
    assert J.dtype == F and r.dtype == F
    return take, J, idx, r


def _products(take, J, idx, r, n):
    """Flat keys and float32 values of every product the reference adds:
    (AtA keys, AtA values, Atb keys, Atb values, r r), pair after pair."""
    J, idx, r = J[take], idx[take], r[take]
    P = (J[:, :, None] * J[:, None, :])
    keys = idx[:, :, None] * n + idx[:, None, :]
    assert P.dtype == F
    return (keys.reshape(-1), P.reshape(-1), idx.reshape(-1),
            (J * r[:, None]).reshape(-1), r * r)


def _exact_scatter(keys, vals, size):
    """out[k] = exactly rounded sum of vals with key k; also sum |vals| and
    the number of terms per key."""
    out = np.zeros(size)
    mag = np.bincount(keys, np.abs(vals).astype(np.float64), size)
    cnt = np.bincount(keys, minlength=size)
    if keys.size:
        order = np.argsort(keys, kind="stable")
        k = keys[order]
        v = vals[order].astype(np.float64).tolist()
        cut = np.flatnonzero(np.diff(k)) + 1
        starts = np.concatenate([[0], cut])
        ends = np.concatenate([cut, [k.size]])
        for s, e in zip(starts.tolist(), ends.tolist()):
            out[k[s]] = math.fsum(v[s:e])
    return out, mag, cnt


def exact_system(take, J, idx, r, n):
    """The full n x n AtA, Atb and residual with exactly rounded float64 sums
    of the float32 products, and per entry sum |terms| and term counts:
    dict(AtA, Atb, residual, mag_A, cnt_A, mag_b, cnt_b, mag_r, cnt_r)."""
    ka, va, kb, vb, rr = _products(take, J, idx, r, n)
    A, mA, cA = _exact_scatter(ka, va, n * n)
    b, mb, cb = _exact_scatter(kb, vb, n)
    return dict(AtA=A.reshape(n, n), Atb=b,
                residual=math.fsum(rr.astype(np.float64).tolist()),
                mag_A=mA.reshape(n, n), cnt_A=cA.reshape(n, n), mag_b=mb,
                cnt_b=cb, mag_r=float(np.abs(rr).astype(np.float64).sum()),
                cnt_r=int(rr.size))


def naive_system(take, J, idx, r, n, reverse=False):
    """The same sums added one after the other in float64, pair after pair
    (reverse: from the last product to the first)."""
    ka, va, kb, vb, rr = _products(take, J, idx, r, n)
    sl = slice(None, None, -1) if reverse else slice(None)
    A = np.zeros(n * n)
    b = np.zeros(n)
    np.add.at(A, ka[sl], va[sl].astype(np.float64))
    np.add.at(b, kb[sl], vb[sl].astype(np.float64))
    res = 0.0
    for v in rr[sl].astype(np.float64).tolist():
        res += v
    return A.reshape(n, n), b, res


def upstream_double_loop(J, idx, r, n):
    """A literal transcription of the reference's loop for the taken pairs,
    float32 products, float64 memory."""
    A = np.zeros((n, n))
    b = np.zeros(n)
    res = 0.0
    for w in range(J.shape[0]):
        for ki in range(60):
            for kj in range(60):
                A[idx[w, ki], idx[w, kj]] += float(F(J[w, ki] * J[w, kj]))
            b[idx[w, ki]] += float(F(J[w, ki] * r[w]))
        res += float(F(r[w] * r[w]))
    return A, b, res


def fast_system(take, J, idx, r, n):
    """Plain float64 sums (bincount order) for the driver."""
    ka, va, kb, vb, rr = _products(take, J, idx, r, n)
    A = np.bincount(ka, va.astype(np.float64), n * n).reshape(n, n)
    b = np.bincount(kb, vb.astype(np.float64), n)
    return A, b, float(rr.astype(np.float64).sum()), int(rr.size)


# ---- regularizer -----------------------------------------------------------

def local_rotation(cov):
    """svd(cov) = U S V^T, R = V U^T with the reference's determinant flip."""
    U, S, Vt = np.linalg.svd(np.asarray(cov, np.float64))
    V = Vt.T
    Ut = U.T.copy()
    R = V @ Ut
    if np.linalg.det(R) < 0:
        Ut[2] = -Ut[2]
        R = V @ Ut
    return R, S


def regularizer(grid_idx, nbs_idx, nbs_mask, init, curr, weight, n_frags,
                anchor_idx, n):
    """-> dict(AtA {n,n}, Atb {n}, residual, sigma: per processed node the
    singular values of its covariance)."""
    init = np.ascontiguousarray(init, F)
    curr = np.ascontiguousarray(curr, F)
    w = F(weight)
    A = np.zeros((n, n))
    b = np.zeros(n)
    res = 0.0
    sigma = {}
    for row, ii in enumerate(np.asarray(grid_idx).tolist()):
        ks = [int(nbs_idx[row, k]) for k in range(6) if nbs_mask[row, k]]
        if len(ks) < 3:
            continue
        cov = np.zeros((3, 3), F)
        for k in ks:
            di = init[ii] - init[k]
            dc = curr[ii] - curr[k]
            cov = cov + di[:, None] * dc[None, :]
        R, S = local_rotation(cov)
        sigma[ii] = S
        R = np.eye(3, dtype=F) if ii == anchor_idx else R.astype(F)
        oi = 6 * n_frags + 3 * ii
        for k in ks:
            di = init[ii] - init[k]
            dc = curr[ii] - curr[k]
            Rd = R[:, 0] * di[0] + R[:, 1] * di[1]
            Rd = Rd + R[:, 2] * di[2]
            lr = dc - Rd
            res += float(w * ((lr[0] * lr[0] + lr[1] * lr[1]) + lr[2] * lr[2]))
            ok = 6 * n_frags + 3 * k
            for a in range(3):
                A[oi + a, oi + a] += float(w)
                A[ok + a, ok + a] += float(w)
                A[oi + a, ok + a] -= float(w)
                A[ok + a, oi + a] -= float(w)
                b[oi + a] += float(w * lr[a])
                b[ok + a] -= float(w * lr[a])
    return dict(AtA=A, Atb=b, residual=res, sigma=sigma)


# ---- the driver ------------------------------------------------------------

def rjt_rows(T_j, x):
    """Rj^T x, each output column sum left to right in float32."""
    t = so.pose_f32(T_j)
    x = np.ascontiguousarray(x, F)
    out = np.empty_like(x)
    for c in range(3):
        v = t[0, c] * x[:, 0] + t[1, c] * x[:, 1]
        out[:, c] = v + t[2, c] * x[:, 2]
    return out


class Grid:
    """Nodes in sorted key order: keys {G,3}, init / curr {G,3} float32."""

    def __init__(self, keys, grid_size, curr=None):
        self.keys = np.asarray(keys, np.int32)
        self.grid_size = grid_size
        self.rank = {tuple(int(v) for v in k): g
                     for g, k in enumerate(self.keys)}
        self.init = (self.keys.astype(F) * F(grid_size)).astype(F)
        self.curr = self.init.copy() if curr is None else \
            np.array(curr, F)
        a = cg.anchor_key(self.keys)
        self.anchor = self.rank[a]
        self.nbs_mask = cg.neighbor_masks(self.keys)
        self.nbs_idx = np.zeros((len(self.keys), 6), np.int64)
        for g, k in enumerate(self.keys):
            for d in range(6):
                if self.nbs_mask[g, d]:
                    self.nbs_idx[g, d] = self.rank[
                        tuple(int(v) for v in (k + cg.DIRECTIONS[d]))]

    def embed(self, points, normals=None):
        """-> (valid, idx {m,8}, vertex ratios, normal ratios)."""
        par = cg.parameterize(points, self.grid_size, self.rank, normals)
        flat = par["keys"].reshape(-1, 3)
        idx = np.array([self.rank[tuple(int(v) for v in k)] for k in flat],
                       np.int64).reshape(-1, 8)
        return par["valid"], idx, par["vertex"], par["normal"]

    def deform(self, idx, vertex, normal=None):
        return cg.deform(self.curr[idx], vertex, normal)


def touch_all(fragments, grid_size):
    keys = [cg.touch(f[0], grid_size)[0] for f in fragments]
    return np.unique(np.concatenate(keys), axis=0)


def edge_arrays(grid, emb_i, emb_j, T_i, T_j):
    """The nine arrays of the seam for an edge from its embedded pairs."""
    ip, rp, rn = emb_i
    iq, rq = emb_j
    Cp, Cn = grid.deform(ip, rp, rn)
    Cq, _ = grid.deform(iq, rq)
    Ri_Cn = so.rotate_rows(T_i, Cn)
    return (so.transform_rows(T_i, Cp), so.transform_rows(T_j, Cq), Cn, Ri_Cn,
            rjt_rows(T_j, Ri_Cn), ip, iq, rp, rq)


def slac_optimize(fragments, poses, edges, grid, max_iterations=5,
                  distance_threshold=0.07, fitness_threshold=0.3,
                  regularizer_weight=1.0, pin_anchor=False):
    """-> dict(status, poses, curr, alignment_losses, regularizer_losses,
    kept, n_corres, n_inliers, skipped); grid.curr is left untouched.

    The reference's system is singular: moving every node by t and
    translating fragment k >= 1 by (R_0 - R_k) t changes no term. pin_anchor
    False is the reference (LU picks the solution its rounding noise selects);
    True is the library's rule, the anchor node's three unknowns taken out
    (identity rows and columns, rhs 0), which leaves a definite system."""
    N = len(fragments)
    G = len(grid.keys)
    n = 6 * N + 3 * G
    grid = Grid(grid.keys, grid.grid_size, grid.curr)
    T = [np.array(p, np.float64) for p in poses]
    sets, emb = [], []
    skipped = 0
    for (i, j, T_ij) in edges:
        cs = so.correspondence_set(fragments[i][0], fragments[j][0], i, j,
                                   T[i], T[j], T_ij, distance_threshold,
                                   fitness_threshold)
        sets.append(cs)
        c = cs["corres"] if cs["kept"] else np.zeros((0, 2), np.int64)
        vi, ip, rp, rn = grid.embed(fragments[i][0][c[:, 0]],
                                    fragments[i][1][c[:, 0]])
        vj, iq, rq, _ = grid.embed(fragments[j][0][c[:, 1]])
        both = vi & vj
        skipped += int((~both).sum())
        ki, kj = both[vi], both[vj]
        emb.append(((ip[ki], rp[ki], rn[ki]), (iq[kj], rq[kj])))
    out = dict(status="ok", kept=[s["kept"] for s in sets],
               n_corres=[s["corres"].shape[0] for s in sets],
               n_inliers=[0] * len(edges), alignment_losses=[],
               regularizer_losses=[], skipped=skipped,
               poses=[t.copy() for t in T], curr=grid.curr.copy())
    for _ in range(max_iterations):
        AtA = np.zeros((n, n))
        Atb = np.zeros(n)
        AtA[np.arange(6), np.arange(6)] = 1.0
        loss = 0.0
        for e, (i, j, _t) in enumerate(edges):
            arrays = edge_arrays(grid, emb[e][0], emb[e][1], T[i], T[j])
            take, J, idx, r = pair_jacobians(*arrays, i, j, N,
                                             distance_threshold)
            A, b, res, cnt = fast_system(take, J, idx, r, n)
            AtA += A
            Atb += b
            loss += res
            out["n_inliers"][e] = cnt
        reg = regularizer(np.arange(G), grid.nbs_idx, grid.nbs_mask,
                          grid.init, grid.curr,
                          F(N) * F(regularizer_weight), N, grid.anchor, n)
        AtA += reg["AtA"]
        Atb += reg["Atb"]
        out["alignment_losses"].append(loss)
        out["regularizer_losses"].append(reg["residual"])
        rhs = -Atb
        if pin_anchor:
            rows = 6 * N + 3 * grid.anchor + np.arange(3)
            AtA[rows, :] = 0.0
            AtA[:, rows] = 0.0
            AtA[rows, rows] = 1.0
            rhs[rows] = 0.0
        try:
            x = np.linalg.solve(AtA, rhs)
        except np.linalg.LinAlgError:
            x = None
        if x is None or not np.all(np.isfinite(x)):
            out["status"] = "singular"
            return out
        T = [so.matmul4(orc.pose_to_transformation(x[6 * k:6 * k + 6]), T[k])
             for k in range(N)]
        grid.curr = (grid.curr + x[6 * N:].reshape(-1, 3).astype(F)).astype(F)
    out["poses"] = T
    out["curr"] = grid.curr
    return out


# ---- the test scene --------------------------------------------------------

def warp(points, k):
    """A smooth displacement of a few centimetres, different per fragment."""
    p = np.asarray(points, np.float64)
    ph = 0.7 * k
    d = np.stack([np.sin(1.3 * p[:, 1] + ph) * np.cos(0.9 * p[:, 2]),
                  np.sin(1.1 * p[:, 2] + 2 * ph) * np.cos(1.2 * p[:, 0]),
                  np.sin(0.8 * p[:, 0] - ph) * np.cos(1.4 * p[:, 1])], 1)
    return (p + 0.03 * d).astype(F)


def make_scene(n_sample=11000, seed=11):
    """Three fragments of about 3000 points of so.make_scene, each warped in
    its own frame; the start poses are slightly wrong. -> (fragments, start
    poses, edges)."""
    frags, _truth, start, edges = so.make_scene(
        n_frag=5, n_sample=n_sample, seed=seed, perturb_deg=0.5,
        perturb_t=0.01)
    edges = [e for e in edges if e[0] < 3 and e[1] < 3]
    frags = [(warp(p, k), n) for k, (p, n) in enumerate(frags[:3])]
    return frags, start[:3], edges


def mean_plane_residual(fragments, poses, edges, sets, grid=None):
    """Mean |point-to-plane residual| over the kept correspondences, the
    fragments deformed by `grid` (a Grid, or None) first."""
    tot, cnt = 0.0, 0
    for e, (i, j, _t) in enumerate(edges):
        c = sets[e]
        if c.shape[0] == 0:
            continue
        pi, ni, pj = fragments[i][0][c[:, 0]], fragments[i][1][c[:, 0]], \
            fragments[j][0][c[:, 1]]
        if grid is not None:
            vi, ip, rp, rn = grid.embed(pi, ni)
            vj, iq, rq, _ = grid.embed(pj)
            assert vi.all() and vj.all()
            pi, ni = grid.deform(ip, rp, rn)
            pj, _ = grid.deform(iq, rq)
        p = so.transform_rows(poses[i], pi).astype(np.float64)
        q = so.transform_rows(poses[j], pj).astype(np.float64)
        nn = so.rotate_rows(poses[i], ni).astype(np.float64)
        tot += float(np.abs(((p - q) * nn).sum(1)).sum())
        cnt += c.shape[0]
    return tot / max(cnt, 1)

# ---- the inputs the CPU and the GPU tests share -------------------------

N_FRAGS, SIDE = 3, 4                      # 3 x 3 x 3 cells, 64 nodes
N_VARS = 6 * N_FRAGS + 3 * SIDE ** 3      # 210


def _node_index(keys):
    keys = np.asarray(keys)
    return (keys[..., 0] * SIDE + keys[..., 1]) * SIDE + keys[..., 2]


ALL_KEYS = {(x, y, z) for x in range(SIDE) for y in range(SIDE)
            for z in range(SIDE)}


def seam_inputs(count, seed, dyadic=False):
    """The nine arrays of an edge (1, 2) in the 64-node grid of cell size 1.
    Half of the pairs sit in one cell (contended entries)."""
    rng = np.random.RandomState(seed)
    if dyadic:
        p = rng.randint(0, 12, (count, 3)) / 4.0
        q = rng.randint(0, 12, (count, 3)) / 4.0
        n = rng.randint(-2, 3, (count, 3)) / 2.0
        cn = rng.randint(-2, 3, (count, 3)) / 2.0
        v = rng.randint(-2, 3, (count, 3)) / 2.0
        dp = rng.randint(-1, 2, (count, 3)) / 8.0
    else:
        p = rng.uniform(0, 3, (count, 3))
        q = np.clip(p + rng.normal(0, 0.05, p.shape), 0, 2.999)
        p[: count // 2] = 1.0 + rng.uniform(0, 1, (count // 2, 3))
        q[: count // 2] = 1.0 + rng.uniform(0, 1, (count // 2, 3))
        n = rng.normal(size=(count, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        cn = rng.normal(size=(count, 3))
        v = rng.normal(size=(count, 3))
        dp = rng.normal(0, 0.04, (count, 3))
    p, q = p.astype(F), q.astype(F)
    pp = cg.parameterize(p, 1.0, ALL_KEYS)
    pq = cg.parameterize(q, 1.0, ALL_KEYS)
    assert pp["valid"].all() and pq["valid"].all()
    return ((q + dp).astype(F), q, cn.astype(F), n.astype(F), v.astype(F),
            _node_index(pp["keys"]).astype(np.int32),
            _node_index(pq["keys"]).astype(np.int32), pp["vertex"],
            pq["vertex"])


def regularizer_cases():
    """(name, grid, curr, masks): the 64-node grid undeformed, rotated with
    smooth noise, with a starved node and with a mirrored neighbourhood."""
    keys = np.array(sorted(ALL_KEYS), np.int32)
    g = Grid(keys, 1.0)
    R = so._rigid(np.random.RandomState(3), 25.0, 0.2)
    rot = (g.init.astype(np.float64) @ R[:3, :3].T + R[:3, 3])
    smooth = 0.05 * np.sin(1.7 * g.init.astype(np.float64)[:, ::-1] + 0.3)
    moved = (rot + smooth).astype(F)
    starved = g.nbs_mask.copy()
    starved[21, 2:] = False                 # an interior node keeps 2
    mirrored = moved.copy()
    mirrored[:, 0] = -mirrored[:, 0]        # det < 0 everywhere
    return [("identity", g, g.init.copy(), g.nbs_mask),
            ("moved", g, moved, g.nbs_mask),
            ("starved", g, moved, starved),
            ("mirrored", g, mirrored, g.nbs_mask)]


GRID_SIZE = 0.375


@functools.lru_cache(maxsize=None)
def scene():
    frags, start, edges = make_scene()
    keys = touch_all(frags, GRID_SIZE)
    return frags, start, edges, Grid(keys, GRID_SIZE)


@functools.lru_cache(maxsize=None)
def oracle_run(iterations=3, pin_anchor=False):
    frags, start, edges, grid = scene()
    return slac_optimize(frags, start, edges, grid, iterations,
                         pin_anchor=pin_anchor)
