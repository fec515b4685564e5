"""The FPFH, Doppler ICP and SLAC fill-in kernels on the MI355X against what
the reference's own compiled kernel bodies returned on the inputs of
tests/_seam_cases.py, as recorded in tests/golden/reference_seams.npz
(written by tests/golden/make_seam_golden.py, pinned to the bodies by
tests/test_seams_vs_ref.py). Reads the inputs and the record only.

Where the record holds a digest instead of the per-pair results (a 1025-pair
alignment case is 3.7 million products), the restatement's per-pair results
are recomputed here, their digest is compared with the recorded one, and only
then are they summed: what the kernel is compared with is, byte for byte, what
the compiled body returned.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _seam_cases as sc
import _slac_nonrigid_oracle as no

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -52
GOLDEN = sc.load_golden()

# The regularizer seam against the recorded FillInSLACRegularizerTermCPU
# results: tolerance 16 x the larger of the restatement's deviation from that
# body measured on the CPU (tests/test_seams_vs_ref.py: the values per case,
# and why the mirrored case's Atb cannot be compared, only its residual) and
# the project's REG_DEVIATION (tests/test_slac_nonrigid_gpu.py).
# Measured on the MI355X, kernel against the record: identity 3.58e-7, moved
# 1.93e-4, starved 1.93e-4, mirrored 0.452; residual of the mirrored case
# 4.28e-7. They equal the restatement's own deviations: the kernel is 3.57e-8
# from the restatement, and the reference's float32 svd3x3 is the rest.
RESTATEMENT_REG_DEVIATION = {"identity": 3.58e-7, "moved": 1.93e-4,
                             "starved": 1.93e-4, "mirrored": 0.452}
RESIDUAL_DEVIATION_MIRRORED = 3.95e-7      # restatement, CPU
REG_DEVIATION = 3.57e-8


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        a.tobytes() == b.tobytes()


def _within(got, exact, mag, cnt, what):
    """exact - bound <= the float64 sum <= exact + bound with bound = count x
    2^-52 x sum |terms| (float64 summation in any order); a float32 result is
    the rounding of that sum, and rounding is monotonic."""
    bound = cnt * EPS * mag
    lo, hi = (exact - bound).astype(got.dtype), (exact + bound).astype(got.dtype)
    bad = ~((got >= lo) & (got <= hi))
    worst = np.abs(got.astype(np.float64) - exact) / np.maximum(mag, 1e-300)
    print("%s: worst |got - exact| / sum|terms| = %.3g" %
          (what, float(worst.max())))
    assert not bad.any(), (what, np.argwhere(bad)[:5])


# ---- FPFH -----------------------------------------------------------------

def run_fpfh(case, form):
    """o3dmi_fpfh_from_neighbors -> (rows, n_fpfh_out); the output is
    prefilled with NaN, so a row the call does not write shows."""
    from open3d_amd import _lib
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    lists, rows, mask = sc.fpfh_form(case, form)
    P, N = _cuda(case["points"]), _cuda(case["normals"])
    idx, d2 = _cuda(lists["idx"]), _cuda(lists["d2"])
    counts = splits = None
    if "splits" in lists:
        splits = _cuda(lists["splits"])
        nn, n_rows = 0, lists["splits"].shape[0] - 1
    else:
        counts = _cuda(lists["counts"])
        n_rows, nn = lists["idx"].shape
    n = case["points"].shape[0]
    m = map_ = None
    n_out = n
    if mask is not None:
        m, map_ = _cuda(mask.astype(np.uint8)), _cuda(rows)
        n_out = int(mask.sum())
    out = torch.full((n_out, 33), float("nan"), dtype=P.dtype, device="cuda")
    got = C.c_int64(-1)
    _lib.check(_lib.lib().o3dmi_fpfh_from_neighbors(
        _lib.ptr(P), _lib.ptr(N), n, TORCH_TO_O3DMI[P.dtype], _lib.ptr(idx),
        _lib.ptr(d2), _lib.ptr(counts), _lib.ptr(splits), nn, n_rows,
        _lib.ptr(m), _lib.ptr(map_), _lib.ptr(out), C.byref(got), stream()),
        "fpfh_from_neighbors")
    torch.cuda.synchronize()
    return out.cpu().numpy(), got.value


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("fixture", ["generic", "lattice"])
def test_fpfh_equals_the_recorded_reference_rows(fixture, dtype):
    """Bit for bit, every row, all three list forms. The build has
    -ffp-contract=off and correctly rounded / and sqrt; acos and atan2 feed
    bin decisions only, which the generic fixture keeps 1e-4 from an edge and
    the lattice puts on exact values."""
    case = sc.fpfh_case(fixture, dtype)
    key = "fpfh/%s/%s/" % (fixture, np.dtype(dtype).name)
    n = case["points"].shape[0]
    for form in sc.FPFH_FORMS:
        want = GOLDEN[key + ("mask" if form == "mask" else "lists")]
        got, n_out = run_fpfh(case, form)
        assert n_out == want.shape[0] == (int(case["mask"].sum())
                                         if form == "mask" else n)
        diff = np.argwhere(got != want)
        assert same(got, want), (form, diff[:5], len(diff))
        cnt = case["counts"][case["mask"]] if form == "mask" \
            else case["counts"]
        assert not got[cnt <= 1].any()
        assert (np.abs(got[cnt > 1]).sum(1) > 0).all()


# ---- Doppler ICP ----------------------------------------------------------

def run_doppler(case, s):
    from open3d_amd import _lib
    from open3d_amd.core import TORCH_TO_O3DMI, stream
    dev = [_cuda(a) for a in case["arrays"]]
    R, r, w, v = (np.ascontiguousarray(a, np.float64) for a in case["prep"])
    sums = torch.full((29,), -7.0, dtype=torch.float64, device="cuda")
    n = case["arrays"][0].shape[0]
    kg, kd = s["kg"], s["kd"]
    _lib.check(_lib.lib().o3dmi_icp_doppler_accumulate(
        *[_lib.ptr(t) for t in dev], n, case["nt"],
        TORCH_TO_O3DMI[dev[0].dtype], _lib.f64p(R), _lib.f64p(r),
        _lib.f64p(w), _lib.f64p(v), C.c_double(sc.PERIOD), int(s["reject"]),
        C.c_double(sc.DOPPLER_THRESHOLD), kg[0], C.c_double(kg[1]),
        C.c_double(kg[2]), kd[0], C.c_double(kd[1]), C.c_double(kd[2]),
        C.c_double(s["lam"]), _lib.ptr(sums), stream()), "doppler_accumulate")
    torch.cuda.synchronize()
    return sums.cpu().numpy()


@pytest.mark.parametrize("s", sc.doppler_settings(), ids=lambda s: s["name"])
def test_doppler_sums_equal_the_recorded_reference_terms(s):
    case = sc.doppler_case(s["n"], s["dtype"])
    key = "doppler/%s/" % s["name"]
    exact, mag, cnt = (GOLDEN[key + k] for k in ("exact", "mag", "count"))
    if key + "terms" in GOLDEN:
        assert same(sc.digest(GOLDEN[key + "terms"]), GOLDEN[key + "digest"])
        e2, m2 = sc.exact_columns(GOLDEN[key + "terms"])
        assert same(e2, exact) and same(m2, mag)
    got = run_doppler(case, s)
    assert got[28] == exact[28] == cnt == (case["arrays"][5] != -1).sum()
    _within(got, exact, mag, float(cnt), s["name"])


# ---- SLAC rigid and alignment terms ----------------------------------------

def _system(n):
    return (torch.zeros((n, n), dtype=torch.float32, device="cuda"),
            torch.zeros(n, dtype=torch.float32, device="cuda"),
            torch.zeros(1, dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("name", list(sc.SLAC_CASES))
def test_rigid_term_equals_the_recorded_reference_pairs(name):
    from open3d_amd import slac
    p, q, n, thr = sc.rigid_inputs(name)
    take, _, A, b, r2 = sc.rigid_products(p, q, n, thr)
    key = "rigid/%s/" % name
    assert same(sc.digest(A, b, r2), GOLDEN[key + "digest"])
    exact, mag = GOLDEN[key + "exact"], GOLDEN[key + "mag"]
    gA, gb, gr = _system(18)
    slac.fill_in_rigid_alignment_term(gA, gb, gr, _cuda(p), _cuda(q),
                                      _cuda(n), *sc.EDGE, thr)
    gA, gb, gr = gA.cpu().numpy(), gb.cpu().numpy(), gr.cpu().numpy()
    assert not gA[:6].any() and not gA[:, :6].any() and not gb[:6].any()
    got = np.concatenate([gA[6:, 6:].reshape(-1), gb[6:], gr])
    cnt = float(take.sum())
    if name == "dyadic":
        assert np.array_equal(got, exact.astype(F))
    _within(got, exact, mag, cnt, "rigid " + name)


@pytest.mark.parametrize("name", list(sc.SLAC_CASES))
def test_alignment_term_equals_the_recorded_reference_pairs(name):
    from open3d_amd import slac
    arrays, thr = sc.slac_case(name)
    take, J, idx, r, P, b, r2 = sc.alignment_products(arrays, thr)
    assert same(sc.digest(P, b, r2), GOLDEN["alignment/%s/digest" % name])
    want = no.exact_system(take, J, idx, r, sc.N_VARS)
    gA, gb, gr = _system(sc.N_VARS)
    st = slac.fill_in_slac_alignment_term_raw(
        gA, gb, gr, *[_cuda(a) for a in arrays], *sc.EDGE, sc.N_FRAGS, thr)
    assert st == 0
    gA, gb, gr = gA.cpu().numpy(), gb.cpu().numpy(), gr.cpu().numpy()
    if name == "dyadic":
        assert {0, 4, 8} <= set(sc.shared_nodes(arrays).tolist())
        assert np.array_equal(gA, want["AtA"].astype(F))
        assert np.array_equal(gb, want["Atb"].astype(F))
        assert gr[0] == F(want["residual"])
        # every sum is exact here, so the reference's float32 running sums
        # are the same numbers
        assert same(sc.digest(gA),
                    GOLDEN["alignment/dyadic/whole_digest"])
        assert np.array_equal(gb, GOLDEN["alignment/dyadic/whole_b"])
        assert np.array_equal(gr, GOLDEN["alignment/dyadic/whole_r"])
    _within(gA, want["AtA"], want["mag_A"], want["cnt_A"], "AtA " + name)
    _within(gb, want["Atb"], want["mag_b"], want["cnt_b"], "Atb " + name)
    _within(gr, np.array([want["residual"]]), np.array([want["mag_r"]]),
            np.array([want["cnt_r"]]), "residual " + name)


# ---- SLAC regularizer ------------------------------------------------------

@pytest.mark.parametrize("case", range(4))
def test_regularizer_term_stays_near_the_recorded_reference(case):
    from open3d_amd import slac
    name, g, curr, masks = no.regularizer_cases()[case]
    key = "regularizer/%s/" % name
    wA = np.zeros(sc.N_VARS * sc.N_VARS, F)
    wA[GOLDEN[key + "at"]] = GOLDEN[key + "values"]
    want = (wA.reshape(sc.N_VARS, sc.N_VARS), GOLDEN[key + "b"],
            float(GOLDEN[key + "r"]))
    gA, gb, gr = _system(sc.N_VARS)
    st = slac.fill_in_slac_regularizer_term_raw(
        gA, gb, gr, _cuda(np.arange(64, dtype=np.int32)),
        _cuda(g.nbs_idx.astype(np.int32)), _cuda(masks), _cuda(g.init),
        _cuda(curr), float(sc.REG_WEIGHT), sc.N_FRAGS, g.anchor)
    assert st == 0
    got = (gA.cpu().numpy(), gb.cpu().numpy(), float(gr.cpu().numpy()[0]))
    dev = sc.regularizer_deviation(got, want)
    print("regularizer %s: deviation from the reference %.3g" % (name, dev))
    assert dev <= 16 * max(RESTATEMENT_REG_DEVIATION[name], REG_DEVIATION)
    assert np.array_equal(got[0], want[0])      # sums of +-weight: exact
    if name == "mirrored":
        rdev = abs(got[2] - want[2]) / want[2]
        print("mirrored: residual deviation %.3g" % rdev)
        assert rdev <= 16 * RESIDUAL_DEVIATION_MIRRORED
