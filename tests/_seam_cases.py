"""The small, deterministic inputs on which the FPFH, Doppler ICP and SLAC
fill-in kernels, their numpy restatements and the reference's compiled bodies
are compared: tests/test_seams_vs_ref.py (restatement against the compiled
body, CPU), tests/golden/make_seam_golden.py (records the compiled body's
results) and tests/test_reference_seams_gpu.py (kernels against the record).
Everything here is numpy; nothing reads oracle/_ref.
"""
import functools
import hashlib
import math

import numpy as np

import _doppler_oracle as dop
import _fpfh_oracle as fo
import _oracle as orc
import _slac_nonrigid_oracle as no
import _slac_oracle as so

F = np.float32
DTYPES = (np.float32, np.float64)


def digest(*arrays):
    """SHA-256 of the arrays' bytes, as uint8 {32}: how the record holds a
    per-pair result that is too large to commit (1025 pairs x 3600 products)."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def exact_columns(terms):
    """{m, k} terms -> (exactly rounded float64 column sums, sum |terms|)."""
    t = np.asarray(terms, np.float64)
    exact = np.array([math.fsum(t[:, k].tolist()) for k in range(t.shape[1])])
    return exact, np.abs(t).sum(0)


# ---- FPFH -----------------------------------------------------------------

def surface(n, seed, dtype):
    """A bumpy closed-ish surface (sum of sines on a sphere): distinctive
    neighbourhoods, analytic outward normals."""
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th = np.arctan2(v[:, 1], v[:, 0])
    ph = np.arccos(np.clip(v[:, 2], -1, 1))
    r = 1.0 + 0.08 * np.sin(5 * th) * np.sin(4 * ph) + 0.05 * np.cos(7 * ph)
    p = v * r[:, None]
    # normals by finite differences of the parametrisation
    e = 1e-6

    def P(t, f):
        rr = 1.0 + 0.08 * np.sin(5 * t) * np.sin(4 * f) + 0.05 * np.cos(7 * f)
        return np.stack([np.sin(f) * np.cos(t), np.sin(f) * np.sin(t),
                         np.cos(f)], 1) * rr[:, None]
    dt_ = (P(th + e, ph) - P(th - e, ph)) / (2 * e)
    dp_ = (P(th, ph + e) - P(th, ph - e)) / (2 * e)
    nrm = np.cross(dp_, dt_)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-300
    nrm *= np.sign((nrm * p).sum(1))[:, None]
    return p.astype(dtype), nrm.astype(dtype)


FPFH_POINTS = 193           # 3 x 64 + 1: both sides of the 64- and 128-row
NN = 24                     # workgroups of SpfhKernel / FpfhKernel
COUNT_CYCLE = (0, 1, 2, 3, 17, 24)
FPFH_SEED = 0               # chosen so that fpfh_validity() holds, see there
MASK_REQUIRED = (0, 63, 64, 127, 128, 192)
BIN_MARGIN = 1e-4           # no bin coordinate this close to an integer
SWAP_MARGIN = 1e-5          # |acos|a1| - acos|a2||: no float / double tie


def _pad(lists, d2s, width, dtype):
    n = len(lists)
    idx = np.full((n, width), -1, np.int32)
    d2 = np.zeros((n, width), dtype)
    counts = np.zeros(n, np.int32)
    for r, (li, ld) in enumerate(zip(lists, d2s)):
        counts[r] = len(li)
        idx[r, :len(li)] = li
        d2[r, :len(li)] = ld
    return idx, d2, counts


def _fpfh_case(points, normals, lists, d2s, width, mask_points):
    """The three list forms of one set of lists: padded, CSR and filtered
    (mask + the sorted union of the masked points and their neighbours)."""
    dt = points.dtype
    idx, d2, counts = _pad(lists, d2s, width, dt)
    splits = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat = np.concatenate([np.asarray(li, np.int32) for li in lists])
    flat_d2 = np.concatenate([np.asarray(ld, dt) for ld in d2s])
    mask = np.zeros(points.shape[0], bool)
    mask[list(mask_points)] = True
    rows = set(int(p) for p in mask_points)
    for p in mask_points:
        rows.update(int(q) for q in lists[p])
    rows = np.array(sorted(rows), np.int64)
    return dict(points=points, normals=normals, idx=idx, d2=d2, counts=counts,
                csr_idx=flat.astype(np.int32), csr_d2=flat_d2.astype(dt),
                splits=splits, mask=mask, map=rows)


def fpfh_form(case, form):
    """-> (list arguments shared by fo.fpfh_from_lists and
    _ref.fpfh_from_lists, list_points or None, mask or None)."""
    if form == "padded":
        return dict(idx=case["idx"], d2=case["d2"],
                    counts=case["counts"]), None, None
    if form == "csr":
        return dict(idx=case["csr_idx"], d2=case["csr_d2"],
                    splits=case["splits"]), None, None
    m = case["map"]
    return dict(idx=case["idx"][m], d2=case["d2"][m],
                counts=case["counts"][m]), m, case["mask"]


FPFH_FORMS = ("padded", "csr", "mask")


def restated_fpfh(case, form, spfh_only=False):
    """fo.fpfh_from_lists on one form. spfh_only: every d2 zeroed, so the
    second pass skips every neighbour and the rows are the SPFH rows (the
    same call gives the compiled body's SPFH rows)."""
    lists, rows, mask = fpfh_form(case, form)
    if spfh_only:
        lists = dict(lists, d2=np.zeros_like(lists["d2"]))
    kw = {}
    if rows is not None:
        kw = dict(list_points=rows, out_points=np.nonzero(mask)[0])
    return fo.fpfh_from_lists(case["points"], case["normals"], **lists, **kw)


@functools.lru_cache(maxsize=None)
def fpfh_generic(dtype_name, seed=FPFH_SEED):
    dt = np.dtype(dtype_name)
    pts, nrm = surface(FPFH_POINTS, seed, dt)
    idx, d2, splits = fo.radius_lists(pts, 1.2)
    lists, d2s = [], []
    for r in range(FPFH_POINTS):
        c = COUNT_CYCLE[r % len(COUNT_CYCLE)]
        s = int(splits[r])
        assert splits[r + 1] - s >= NN and idx[s] == r
        lists.append(idx[s:s + c])
        d2s.append(d2[s:s + c])
    rng = np.random.RandomState(7)
    rest = np.setdiff1d(np.arange(FPFH_POINTS), MASK_REQUIRED)
    masked = sorted(MASK_REQUIRED + tuple(
        int(v) for v in rng.choice(rest, 40 - len(MASK_REQUIRED), False)))
    return _fpfh_case(pts, nrm, lists, d2s, NN, masked)


# The lattice: coordinates in units of 2^-3, axis-aligned unit (or zero)
# normals. Every product, sum and difference below is exact in both dtypes;
# sqrt and / are correctly rounded on every side.
_X, _Y, _Z, _O = (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)
_NEG = lambda v: tuple(-c for c in v)                        # noqa: E731
LATTICE = [
    ((0, 0, 0), _Z),         # 0
    ((1, 0, 0), _Z),         # 1  equal normals with 0
    ((0, 0, 0), _X),         # 2  coincident with 0
    ((0, 0, 2), _Z),         # 3  dp parallel to 0's normal: v_norm == 0
    ((2, 0, 0), _NEG(_Y)),   # 4  f1 == +1 from 0 (bin 11 clamps to 10)
    ((4, 0, 0), _Y),         # 5  f1 == -1 from 0 (bin 0)
    ((0, 1, 0), _NEG(_Z)),   # 6  antiparallel to 0: atan2(+-0, -1)
    ((0, 2, 0), _O),         # 7  zero normal
    ((1, 1, 0), _X),         # 8  diagonal: the normals swap roles
    ((3, 4, 0), _Y),         # 9  |dp| = 5/8, swap
    ((0, 0, -1), _Z),        # 10 dp antiparallel to 0's normal
    ((1, 0, 1), _NEG(_X)),   # 11
    ((2, 2, 2), _Y),         # 12 all its neighbours have count <= 1
    ((0, 3, 0), _Y),         # 13 from 0: swapped normal parallel to dp
    ((2, 2, 1), _NEG(_Z)),   # 14 from 12: the same (v_norm == 0 after swap)
    ((-1, 0, 0), _NEG(_Z)),  # 15 antiparallel to 0 on the other side
]
# list rows: position 0 is skipped by both passes whatever it holds
LATTICE_LISTS = {
    0: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 15, 11],   # 2: d2 == 0
    1: [4, 0, 5, 8, 9, 11],          # position 0 is not the point itself
    2: [2, 0, 1, 8, 6],              # 0 coincident, its d2 hand-set to 1/64
    3: [3, 0, 11, 10],
    4: [4, 1, 5, 0, 6],
    5: [5, 4, 9],
    6: [6, 0, 15, 7, 8],
    7: [7, 6, 0, 13],                # the row of the zero normal
    8: [8, 0, 1, 6, 2],
    9: [9, 5, 4, 8],
    10: [10, 0, 3],
    11: [11, 1, 3, 0],
    12: [12, 13, 14, 15],            # sum[g] == 0: 13, 14, 15 have no SPFH
    13: [13],
    14: [14],
    15: [],
}
LATTICE_MASK = (0, 2, 7, 12, 15)


@functools.lru_cache(maxsize=None)
def fpfh_lattice(dtype_name):
    dt = np.dtype(dtype_name)
    pts = (np.array([p for p, _ in LATTICE], np.float64) / 8.0).astype(dt)
    nrm = np.array([n for _, n in LATTICE], np.float64).astype(dt)
    lists, d2s = [], []
    for r in range(len(LATTICE)):
        li = np.array(LATTICE_LISTS[r], np.int32)
        d = pts[li] - pts[r] if li.size else np.zeros((0, 3), dt)
        d2 = (d * d).sum(1).astype(dt)          # exact on the lattice
        if r == 2:
            d2[1] = dt.type(1.0 / 64.0)         # coincident, d2 != 0
        lists.append(li)
        d2s.append(d2)
    assert d2s[0][2] == 0
    return _fpfh_case(pts, nrm, lists, d2s, 14, LATTICE_MASK)


def fpfh_case(fixture, dtype):
    name = np.dtype(dtype).name
    return fpfh_generic(name) if fixture == "generic" else fpfh_lattice(name)


def fpfh_pairs(case):
    """(row point, neighbour) of every pair the SPFH pass forms."""
    a, b = [], []
    for r in range(case["idx"].shape[0]):
        for i in range(1, int(case["counts"][r])):
            a.append(r)
            b.append(int(case["idx"][r, i]))
    return np.array(a, np.int64), np.array(b, np.int64)


def fpfh_validity(case):
    """-> (smallest distance of a bin coordinate from an integer, smallest
    |acos|a1| - acos|a2|| in float64, number of pairs whose swap decision
    differs between the point dtype and float64). The generic fixture's seed
    keeps these at >= BIN_MARGIN, >= SWAP_MARGIN and 0, so that neither one
    ulp of acos / atan2 nor the precision of the swap test can move a pair to
    another bin on any side of the comparison."""
    a, b = fpfh_pairs(case)
    P, N, dt = case["points"], case["normals"], case["points"].dtype
    f = fo.pair_features(P[a], N[a], P[b], N[b], dt)
    c = np.stack(fo.bin_coords_v(f), 1)
    a1, a2 = fo.pair_angles(P[a], N[a], P[b], N[b], dt)
    narrow = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
    w1 = np.arccos(np.abs(a1).astype(np.float64))
    w2 = np.arccos(np.abs(a2).astype(np.float64))
    return (float(np.abs(c - np.round(c)).min()), float(np.abs(w1 - w2).min()),
            int((narrow != (w1 > w2)).sum()))


# ---- Doppler ICP ----------------------------------------------------------

V_LEVER = np.array([[0.0, -1.0, 0.0, 0.4], [1.0, 0.0, 0.0, -0.2],
                    [0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
DOPPLER_SIZES = (1, 64, 65, 1025)
DOPPLER_THRESHOLD = 0.25      # a power of two: planted errors hit it exactly
PERIOD = 0.1
KERNELS = {dop.L2: (dop.L2, 1.0, 1.0), dop.L1: (dop.L1, 1.0, 1.0),
           dop.HUBER: (dop.HUBER, 0.03, 1.0),
           dop.CAUCHY: (dop.CAUCHY, 0.05, 1.0), dop.GM: (dop.GM, 0.05, 1.0),
           dop.TUKEY: (dop.TUKEY, 0.05, 1.0),
           dop.GENERALIZED: (dop.GENERALIZED, 0.05, 1.0)}


@functools.lru_cache(maxsize=None)
def doppler_case(n, dtype_name):
    """n source rows against 3 n / 4 + 5 target points, about 20 % of the rows
    without a correspondence, a lever arm and a quarter-turn R_S_to_V; Doppler
    errors of 0.3 sigma around a threshold of 0.25, and (n >= 64) three pairs
    whose error is the threshold exactly. -> dict(arrays, nt, prep, at)."""
    dt = np.dtype(dtype_name)
    rng = np.random.default_rng(1000 + n)
    nt = 3 * n // 4 + 5
    tgt = rng.uniform(-3, 3, (nt, 3))
    tn = rng.standard_normal((nt, 3))
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    corr = rng.integers(0, nt, n).astype(np.int64)
    src = tgt[corr] + 0.05 * rng.standard_normal((n, 3))
    corr[rng.random(n) < 0.2] = -1
    if n == 1:
        corr[0] = nt - 1
    dirs = src / np.linalg.norm(src, axis=1, keepdims=True)
    T = orc.pose_to_transformation([0.02, -0.03, 0.01, 0.1, -0.05, 0.07])
    prep = dop.host_prepare(V_LEVER, T, PERIOD, dt)
    dirs = dirs.astype(dt)
    pred = dop.predicted_doppler(dirs, *prep)
    dops = (pred + (0.3 * rng.standard_normal(n)).astype(dt)).astype(dt)
    at = []
    if n >= 64:
        thr = dt.type(DOPPLER_THRESHOLD)
        for k in np.nonzero(corr >= 0)[0]:
            for sign in (1, -1):
                d = dt.type(pred[k] + sign * thr)
                if abs(np.float64(dt.type(d - pred[k]))) == DOPPLER_THRESHOLD:
                    dops[k] = d
                    at.append(int(k))
                    break
            if len(at) == 3:
                break
        assert len(at) == 3
    arrays = [np.ascontiguousarray(a.astype(dt))
              for a in (src, dops, dirs, tgt, tn)] + [corr]
    return dict(arrays=arrays, nt=nt, prep=prep, at=at)


def doppler_errors(case):
    """|Doppler error| of every row, as the rejection test sees it."""
    a = case["arrays"]
    pred = dop.predicted_doppler(a[2], *case["prep"])
    return np.abs((a[1] - pred).astype(np.float64))


def _setting(name, n, dt, kg, kd, reject=False, lam=0.01):
    return dict(name="%s_n%d_%s" % (name, n, np.dtype(dt).name), n=n,
                dtype=np.dtype(dt).name, kg=KERNELS[kg], kd=KERNELS[kd],
                reject=reject, lam=lam)


def doppler_settings():
    """The recorded cases: every size and dtype plain and with rejection; at
    65 pairs the seven equal kernel pairs, (Huber, Tukey), (Tukey, L1) and
    lambda_doppler 0 and 1."""
    out = []
    for dt in DTYPES:
        for n in DOPPLER_SIZES:
            out.append(_setting("l2", n, dt, dop.L2, dop.L2))
            out.append(_setting("reject", n, dt, dop.TUKEY, dop.TUKEY, True))
        for m in range(1, 7):
            out.append(_setting("equal%d" % m, 65, dt, m, m))
        out.append(_setting("huber_tukey", 65, dt, dop.HUBER, dop.TUKEY))
        out.append(_setting("tukey_l1", 65, dt, dop.TUKEY, dop.L1))
        for lam in (0.0, 1.0):
            out.append(_setting("lambda%d" % lam, 65, dt, dop.L2, dop.TUKEY,
                                True, lam))
    return out


def restated_doppler_terms(case, s):
    """-> {n, 29} of the point dtype, one row per source row (zeros where
    there is no correspondence), from _doppler_oracle.pair_terms, each row
    added to zeros."""
    a = case["arrays"]
    A, _ = dop.pair_terms(*a, *case["prep"], PERIOD, s["reject"],
                          DOPPLER_THRESHOLD, s["kg"], s["kd"], s["lam"])
    out = np.zeros((a[0].shape[0], 29), a[0].dtype)
    out[a[5] != -1] += A        # summed into zeros, as the body does: -0 -> 0
    return out


# ---- SLAC fill-ins ----------------------------------------------------------

N_FRAGS, N_VARS = no.N_FRAGS, no.N_VARS
EDGE = (1, 2)
SLAC_CASES = {"1": (1, 101, False, 0.05), "255": (255, 355, False, 0.05),
              "1025": (1025, 1125, False, 0.05),
              "dyadic": (255, 5, True, 0.0625)}


@functools.lru_cache(maxsize=None)
def slac_case(name):
    """-> (the nine arrays of no.seam_inputs, threshold)."""
    count, seed, dyadic, threshold = SLAC_CASES[name]
    return no.seam_inputs(count, seed, dyadic=dyadic), threshold


def shared_nodes(arrays):
    """Per pair, how many of p's eight grid nodes are also q's."""
    ip, iq = arrays[5], arrays[6]
    return np.array([len(set(a.tolist()) & set(b.tolist()))
                     for a, b in zip(ip, iq)])


def relabelled(arrays):
    """The same pairs with p's nodes called 0..7 and q's 8..15: with distinct
    labels a pair's 60 x 60 block holds every product J_a J_b on its own."""
    a = list(arrays)
    m = a[0].shape[0]
    a[5] = np.tile(np.arange(8, dtype=np.int32), (m, 1))
    a[6] = np.tile(np.arange(8, 16, dtype=np.int32), (m, 1))
    return tuple(a)


def alignment_products(arrays, threshold):
    """-> (take, J {m,60}, idx {m,60}, r {m}, P {m,60,60} = J_a J_b,
    b {m,60} = J_a r, r2 {m}), all float32, rows of pairs beyond the threshold
    zeroed in P, b and r2 (such a pair adds nothing)."""
    take, J, idx, r = no.pair_jacobians(*arrays, *EDGE, N_FRAGS, threshold)
    # "+ 0": each product as the body leaves it after adding it to a zero
    P = J[:, :, None] * J[:, None, :] + F(0)
    b = J * r[:, None] + F(0)
    r2 = r * r
    P[~take], b[~take], r2[~take] = 0, 0, 0
    assert P.dtype == F and b.dtype == F and r2.dtype == F
    return take, J, idx, r, P, b, r2


def alignment_pair_f32(J, idx, r, n):
    """One taken pair added into a zeroed float32 system in the reference's
    loop order (ki outer, kj inner): where p and q share grid nodes several
    products meet in one entry and the order of the float32 adds shows."""
    A = np.zeros(n * n, F)
    b = np.zeros(n, F)
    keys = (idx[:, None] * n + idx[None, :]).reshape(-1)
    np.add.at(A, keys, (J[:, None] * J[None, :]).reshape(-1))
    np.add.at(b, idx, J * r)
    return A.reshape(n, n), b, F(r * r)


def alignment_whole_f32(take, J, idx, r, n):
    """Every taken pair, in order, into one float32 system: the reference's
    result on one thread."""
    J, idx, r = J[take], idx[take], r[take]
    A = np.zeros(n * n, F)
    b = np.zeros(n, F)
    res = np.zeros(1, F)
    keys = (idx[:, :, None] * n + idx[:, None, :]).reshape(-1)
    np.add.at(A, keys, (J[:, :, None] * J[:, None, :]).reshape(-1))
    np.add.at(b, idx.reshape(-1), (J * r[:, None]).reshape(-1))
    for v in (r * r):
        res[0] = res[0] + v
    return A.reshape(n, n), b, res


def rigid_inputs(name):
    """Ti_ps, Tj_qs, Ri_normal_ps of a SLAC case and its threshold."""
    arrays, threshold = slac_case(name)
    return arrays[0], arrays[1], arrays[3], threshold


def rigid_products(p, q, n, threshold):
    """-> (take, terms {m,28}, A {m,12,12}, b {m,12}, r2 {m}) float32: each
    pair's 12 x 12 block of the Jacobian (J, -J), rhs and squared residual,
    zero for a pair beyond the threshold."""
    take, terms, J, r = so.pair_terms(p, q, n, threshold)
    J12 = np.concatenate([J, -J], 1)
    A = J12[:, :, None] * J12[:, None, :] + F(0)    # added to a zero
    b = J12 * r[:, None] + F(0)
    r2 = r * r
    A[~take], b[~take], r2[~take] = 0, 0, 0
    return take, terms, A, b, r2


REG_WEIGHT = F(3.0)


def regularizer_deviation(got, want):
    """Largest deviation of (AtA, Atb, residual) relative to the largest
    entry: the measure of tests/test_slac_nonrigid_gpu.py."""
    A, b, res = got
    wA, wb, wr = (np.asarray(want[0], np.float64),
                  np.asarray(want[1], np.float64), float(want[2]))
    return float(max(np.abs(A - wA).max() / np.abs(wA).max(),
                     np.abs(b - wb).max() / max(np.abs(wb).max(), 1.0),
                     abs(float(res) - wr) / max(wr, 1.0)))


# ---- the record ------------------------------------------------------------

def load_golden():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "reference_seams.npz")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
