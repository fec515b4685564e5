"""The gather-and-accumulate frame of icp.hip at its edges: every public entry
point that gathers by correspondence, both dtypes, at a lone pair and at one
full grid plus a second trip of the grid-stride loop.

The gather kernels run at most 2 * 256 workgroups of 256 threads = 131 072
threads, so N_BIG = 131 072 + 257 rows make threads 0..256 of the first
workgroup (its first wave whole, one thread of the next) go round a second
time; no other direct test of these kernels is that large. Every seventh row
is -1, the others are seeded indices into a target of NT points. Each entry is
held to the oracle and the tolerance of its own parity test (named at each
test); the pair count is exact and a second call returns the same bytes.

No pair is left out of any comparison: on the CPU the oracles give finite sums
at these sizes and seeds, and the generalized estimator's covariances leave
slot 29 (pairs that cannot be whitened) at 0 under both of the oracle's routes
to the root."""
import ctypes as C

import numpy as np
import pytest
import torch

import _doppler_oracle as dop
import _gicp_oracle as gicp
import _oracle as orc
from test_doppler_gpu import V_LEVER
from test_gicp_cpu import K

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
N_BIG = 2 * 256 * 256 + 257
SIZES = (1, N_BIG)
NT = 4001
DTYPES = (np.float32, np.float64)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib, registration
    return _lib, registration


def _f64p(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(
        C.POINTER(C.c_double))


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_CASES = {}


def case(n, dtype):
    """n source rows against NT target points, the pairs a few centimetres
    apart, row i without a correspondence where i % 7 == 6 (rows 0 and n - 1
    of both sizes have one); every estimator's attributes. Shared, read-only."""
    key = (n, np.dtype(dtype).name)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 + n)
    tgt = rng.uniform(-3, 3, (NT, 3))
    tn = _unit(rng.standard_normal((NT, 3)))
    corr = rng.integers(0, NT, n).astype(np.int64)
    src = tgt[corr] + 0.05 * rng.standard_normal((n, 3))
    sn = _unit(tn[corr] + 0.1 * rng.standard_normal((n, 3)))
    corr[6::7] = -1
    c = dict(n=n, corr=corr, pairs=int((corr >= 0).sum()))
    f = lambda a: np.ascontiguousarray(a.astype(dtype))  # noqa: E731
    c.update(src=f(src), tgt=f(tgt), tn=f(tn), sn=f(sn))
    # coloured: colours in [0, 1], gradients of a few units per metre
    c.update(sc=f(rng.uniform(0, 1, (n, 3))), tc=f(rng.uniform(0, 1, (NT, 3))),
             tg=f(rng.standard_normal((NT, 3))))
    # Doppler (the recipe of test_doppler_gpu._accumulate_case)
    dirs = f(_unit(src))
    T = orc.pose_to_transformation([0.02, -0.03, 0.01, 0.1, -0.05, 0.07])
    c["prep"] = dop.host_prepare(V_LEVER, T, 0.1, dtype)
    c["dirs"] = dirs
    c["dops"] = f(dop.predicted_doppler(dirs, *c["prep"]) +
                  (0.3 * rng.standard_normal(n)).astype(dtype))
    # generalized (the recipe of _gicp_oracle.accumulate_case)
    c["cs"] = gicp.covariances_from_normals(f(sn @ gicp.r_source()), 1e-3)
    c["ct"] = gicp.covariances_from_normals(c["tn"], 1e-3)
    _CASES[key] = c
    return c


def _dev(c, *names):
    """The case's arrays on the device, uploaded once."""
    d = c.setdefault("dev", {})
    for k in names:
        if k not in d:
            d[k] = torch.from_numpy(c[k]).cuda()
    return [d[k] for k in names]


def _twice(_lib, n_sums, call):
    """call(sums) -> status, on a sentinel-filled buffer, twice: the same
    bytes both times -> the sums."""
    got = []
    for _ in range(2):
        sums = torch.full((n_sums,), -7.0, dtype=torch.float64, device="cuda")
        _lib.check(call(sums), "accumulate")
        torch.cuda.synchronize()
        got.append(sums.cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes()
    return got[0]


def _dt(t):
    from open3d_amd.core import TORCH_TO_O3DMI
    return TORCH_TO_O3DMI[t.dtype]


def _moments(c):
    """The 16 sums of o3dmi_icp_p2point_accumulate in float64 (numpy)."""
    m = c["corr"] >= 0
    s64 = c["src"][m].astype(np.float64)
    t64 = c["tgt"][c["corr"][m]].astype(np.float64)
    return np.concatenate([s64.sum(0), t64.sum(0), (t64.T @ s64).reshape(-1),
                           [m.sum()]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_p2plane(n, dtype):
    """test_icp_gpu.test_p2plane_accumulate_parity: 1e-9 of the largest sum."""
    _lib, _ = _gpu()
    from open3d_amd.core import stream
    c = case(n, dtype)
    kernel = (2, 0.05, 1.0)
    s, t, tn, corr = _dev(c, "src", "tgt", "tn", "corr")
    got = _twice(_lib, 29, lambda out: _lib.lib().o3dmi_icp_p2plane_accumulate(
        _lib.ptr(s), _lib.ptr(t), _lib.ptr(tn), _lib.ptr(corr), n, _dt(s),
        kernel[0], C.c_double(kernel[1]), C.c_double(kernel[2]), _lib.ptr(out),
        stream()))
    want = orc.p2plane_accumulate(c["src"], c["tgt"], c["tn"], c["corr"],
                                  *kernel, accumulate_double=True)
    print(n, "max |diff| / scale", np.abs(got - want).max() / np.abs(want).max())
    assert got[28] == want[28] == c["pairs"]
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_p2point(n, dtype):
    """test_icp_gpu.test_p2point_accumulate_and_rt_parity: the float64 moments
    in numpy, rtol 1e-12, atol 1e-9."""
    _lib, _ = _gpu()
    from open3d_amd.core import stream
    c = case(n, dtype)
    s, t, corr = _dev(c, "src", "tgt", "corr")
    got = _twice(_lib, 16, lambda out: _lib.lib().o3dmi_icp_p2point_accumulate(
        _lib.ptr(s), _lib.ptr(t), _lib.ptr(corr), n, _dt(s), _lib.ptr(out),
        stream()))
    assert got[15] == c["pairs"]
    assert np.allclose(got, _moments(c), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_information(n, dtype):
    """test_icp_gpu.test_information_matrix_parity's kernel seam: rtol 1e-12,
    atol 1e-9. The 21 sums carry no count: entry 9 (G_33) is a 1 per pair."""
    _lib, _ = _gpu()
    from open3d_amd.core import stream
    c = case(n, dtype)
    t, corr = _dev(c, "tgt", "corr")
    got = _twice(
        _lib, 21, lambda out: _lib.lib().o3dmi_icp_information_accumulate(
            _lib.ptr(t), _lib.ptr(corr), n, _dt(t), _lib.ptr(out), stream()))
    want = orc.information_accumulate(c["tgt"], c["corr"],
                                      accumulate_double=True)
    assert got[9] == want[9] == c["pairs"]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_symmetric(n, dtype):
    """test_icp_gpu.test_symmetric_accumulate_parity: rtol 1e-11, atol 1e-9,
    about the means of the matched points in the clouds' dtype."""
    _lib, _ = _gpu()
    from open3d_amd.core import stream
    c = case(n, dtype)
    kernel = (3, 0.05, 1.0)
    mom = _moments(c)
    ms = (mom[0:3] / mom[15]).astype(dtype).astype(np.float64)
    mt = (mom[3:6] / mom[15]).astype(dtype).astype(np.float64)
    s, sn, t, tn, corr = _dev(c, "src", "sn", "tgt", "tn", "corr")
    got = _twice(
        _lib, 29, lambda out: _lib.lib().o3dmi_icp_symmetric_accumulate(
            _lib.ptr(s), _lib.ptr(sn), _lib.ptr(t), _lib.ptr(tn),
            _lib.ptr(corr), n, _dt(s), _f64p(ms), _f64p(mt), kernel[0],
            C.c_double(kernel[1]), C.c_double(kernel[2]), _lib.ptr(out),
            stream()))
    want = orc.symmetric_accumulate(c["src"], c["tgt"], c["sn"], c["tn"],
                                    c["corr"], ms, mt, *kernel,
                                    accumulate_double=True)
    assert got[28] == want[28] == c["pairs"]
    assert np.allclose(got, want, rtol=1e-11, atol=1e-9)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_colored(n, dtype):
    """test_icp_gpu.test_colored_accumulate_parity: rtol 1e-11, atol 1e-9."""
    _lib, _ = _gpu()
    from open3d_amd.core import stream
    c = case(n, dtype)
    kernel = (5, 0.05, 1.0)
    names = ("src", "sc", "tgt", "tn", "tc", "tg", "corr")
    dev = _dev(c, *names)
    got = _twice(_lib, 29, lambda out: _lib.lib().o3dmi_icp_colored_accumulate(
        *[_lib.ptr(t) for t in dev], n, _dt(dev[0]), C.c_double(0.968),
        kernel[0], C.c_double(kernel[1]), C.c_double(kernel[2]), _lib.ptr(out),
        stream()))
    want = orc.colored_accumulate(*[c[k] for k in names], 0.968, *kernel,
                                  accumulate_double=True)
    assert got[28] == want[28] == c["pairs"]
    assert np.allclose(got, want, rtol=1e-11, atol=1e-9)


DOPPLER = dict(period=0.1, reject=True, threshold=0.3,
               kg=(dop.CAUCHY, 0.05, 1.0), kd=(0, 1.0, 1.0), lam=0.01)
DOPPLER_NAMES = ("src", "dops", "dirs", "tgt", "tn", "corr")


def _doppler(_lib, dev, n, prep, sums):
    from open3d_amd.core import stream
    p = DOPPLER
    R, r, w, v = (np.asarray(a, np.float64) for a in prep)
    return _lib.lib().o3dmi_icp_doppler_accumulate(
        *[_lib.ptr(t) for t in dev], n, NT, _dt(dev[0]), _f64p(R), _f64p(r),
        _f64p(w), _f64p(v), C.c_double(p["period"]), int(p["reject"]),
        C.c_double(p["threshold"]), p["kg"][0], C.c_double(p["kg"][1]),
        C.c_double(p["kg"][2]), p["kd"][0], C.c_double(p["kd"][1]),
        C.c_double(p["kd"][2]), C.c_double(p["lam"]), _lib.ptr(sums), stream())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_doppler(n, dtype):
    """test_doppler_gpu.test_doppler_accumulate_parity's "reject" setting:
    rtol 1e-11, atol 1e-9; a rejected pair stays in the count."""
    _lib, _ = _gpu()
    c = case(n, dtype)
    dev = _dev(c, *DOPPLER_NAMES)
    got = _twice(_lib, 29,
                 lambda out: _doppler(_lib, dev, n, c["prep"], out))
    p = DOPPLER
    args = [c[k] for k in DOPPLER_NAMES] + list(c["prep"]) + [
        p["period"], p["reject"], p["threshold"], p["kg"], p["kd"], p["lam"]]
    want = dop.accumulate(*args)
    assert got[28] == want[28] == c["pairs"]
    assert np.allclose(got, want, rtol=1e-11, atol=1e-9)
    if n == N_BIG:
        _, rejected = dop.pair_terms(*args)
        assert 0 < rejected.sum() < rejected.size


GICP_KERNEL = gicp.SETTINGS["huber"]
GICP_NAMES = ("src", "cs", "tgt", "ct", "corr")


def _generalized(_lib, dev, n, sums):
    from open3d_amd.core import stream
    return _lib.lib().o3dmi_icp_generalized_accumulate(
        *[_lib.ptr(t) for t in dev], n, NT, _dt(dev[0]),
        _f64p(gicp.r_source()), GICP_KERNEL[0], C.c_double(GICP_KERNEL[1]),
        C.c_double(GICP_KERNEL[2]), _lib.ptr(sums), stream())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_generalized(n, dtype):
    """test_gicp_gpu.test_generalized_accumulate_parity: per entry within
    K 2^-52 sum |term| (test_gicp_cpu derives K); every pair is whitened."""
    _lib, _ = _gpu()
    c = case(n, dtype)
    dev = _dev(c, *GICP_NAMES)
    got = _twice(_lib, 32, lambda out: _generalized(_lib, dev, n, out))
    want, abs_sums = gicp.accumulate(*[c[k] for k in GICP_NAMES],
                                     gicp.r_source(), GICP_KERNEL)
    assert want[29] == 0
    assert got[28] == want[28] == c["pairs"]
    assert got[29] == 0 and got[30] == 0 and got[31] == 0
    bound = K * 2.0 ** -52 * abs_sums
    diff = np.abs(got[:29] - want[:29])
    with np.errstate(all="ignore"):
        print(n, "largest |diff| / bound",
              np.where(bound > 0, diff / bound, 0.0).max())
    assert np.all(diff <= bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_compute_rmse(n, dtype):
    """o3dmi_registration_compute_rmse, the way to ResidualSquaresKernel, and
    its generalized form (the kRmse kernel).
    Point-to-plane and point-to-point: the squares formed in the clouds' dtype
    and summed in float64 by numpy -- the kernel's terms in another order of
    float64 additions, rtol 1e-12 as for the point-to-point moments.
    Point-to-plane also against _oracle.p2plane_rmse within 1e-6
    (test_icp_gpu.test_compute_rmse_goldens_through_gpu), except Float32 at
    N_BIG: there the oracle adds 337 704 squares one after the other in
    Float32 and is itself 5.0e-6 away from the float64 sum of its own terms
    (0.0500438682 against 0.0500489057, on the CPU).
    Generalized: _gicp_oracle.compute_rmse within 1e-12 of it
    (test_gicp_gpu.test_compute_rmse_generalized)."""
    _lib, reg = _gpu()
    c = case(n, dtype)
    s, t, tn, corr, cs, ct = _dev(c, "src", "tgt", "tn", "corr", "cs", "ct")

    def twice(est, normals, **kw):
        a = reg.compute_rmse(est, s, t, normals, corr, **kw)
        assert a == reg.compute_rmse(est, s, t, normals, corr, **kw)
        return a
    m = c["corr"] >= 0
    e = c["src"][m] - c["tgt"][c["corr"][m]]
    for est, normals in ((reg.TransformationEstimationPointToPoint(), None),
                         (reg.TransformationEstimationPointToPlane(), tn)):
        r = e if normals is None else e * c["tn"][c["corr"][m]]
        want = np.sqrt((r * r).astype(np.float64).sum() / c["pairs"])
        got = twice(est, normals)
        print(n, type(est).__name__, got, "relative difference",
              abs(got - want) / want)
        assert abs(got - want) <= 1e-12 * want
    if not (n == N_BIG and dtype == np.float32):
        assert abs(got - orc.p2plane_rmse(c["src"], c["tgt"], c["tn"],
                                          c["corr"])) < 1e-6
    want = gicp.compute_rmse(*[c[k] for k in GICP_NAMES])
    got = twice(reg.TransformationEstimationForGeneralizedICP(), None,
                source_covariances=cs, target_covariances=ct)
    print(n, "generalized", got, "relative difference",
          abs(got - want) / want)
    assert abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["doppler", "generalized"])
def test_range_check_in_the_second_trip(entry, dtype):
    """An index outside the target in row N_BIG - 1 alone -- a row only a
    second-trip thread reads: INVALID_ARG, and the sentinel-filled sums are
    untouched. The same row at -1: OK."""
    _lib, _ = _gpu()
    c = case(N_BIG, dtype)
    names = DOPPLER_NAMES if entry == "doppler" else GICP_NAMES
    n_sums = 29 if entry == "doppler" else 32
    dev = list(_dev(c, *names))

    def run(last):
        corr = c["corr"].copy()
        corr[N_BIG - 1] = last
        dev[-1] = torch.from_numpy(corr).cuda()
        sums = torch.full((n_sums,), -7.0, dtype=torch.float64, device="cuda")
        st = (_doppler(_lib, dev, N_BIG, c["prep"], sums)
              if entry == "doppler" else _generalized(_lib, dev, N_BIG, sums))
        torch.cuda.synchronize()
        return st, sums.cpu().numpy()
    for bad in (NT, -2):
        st, sums = run(bad)
        assert st == INVALID_ARG, bad
        assert b"out of range" in _lib.lib().o3dmi_last_error()
        assert np.array_equal(sums, np.full(n_sums, -7.0)), bad
    st, sums = run(-1)
    assert st == 0
    assert sums[28] == c["pairs"] - 1
