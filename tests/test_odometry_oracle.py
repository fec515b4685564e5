"""Pins the RGB-D odometry oracle (oracle/odometry_oracle.cpp):

1. against the golden vectors in the reference's own test-suite
   (cpp/tests/t/geometry/Image.cpp) -- including the IPP-path goldens for the
   filters that have no in-tree arithmetic;
2. bit for bit against the reference's own kernel bodies (ImageCPU.cpp,
   RGBDOdometryCPU.cpp compiled through oracle/ref_shim -> oracle/_ref).
"""
import numpy as np
import pytest

import _odometry_cases as cases
import _oracle as orc
import _ref as ref
from open3d_amd import synthetic

needs_ref = pytest.mark.skipif(not ref.available(),
                               reason="oracle/_ref not built")
NAN = float("nan")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 1. goldens of cpp/tests/t/geometry/Image.cpp
# ---------------------------------------------------------------------------
def test_depth_to_vertex_normal_maps_golden():
    # Image.cpp:829-876
    depth = np.array([0, 1, 2, 1, 0, 0, 2, 4, 2, 0, 0, 3, 6, 3, 29, 0, 2, 4, 2,
                      0, 0, 1, 2, 1, 0], np.uint16).reshape(5, 5)
    clipped_ref = np.array([0.0, 0.1, 0.2, 0.1, 0.0, 0.0, 0.2, 0.4, 0.2, 0.0,
                            0.0, 0.3, 0.6, 0.3, 0.0, 0.0, 0.2, 0.4, 0.2, 0.0,
                            0.0, 0.1, 0.2, 0.1, 0.0], np.float32).reshape(5, 5)
    K = np.array([[1, 0, 2], [0, 1, 2], [0, 0, 1]], np.float64)
    vertex_ref = np.array([
        0.0, 0.0, 0.0, -0.1, -0.2, 0.1, 0.0, -0.4, 0.2, 0.1, -0.2, 0.1, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, -0.2, -0.2, 0.2, 0.0, -0.4, 0.4, 0.2, -0.2, 0.2, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, -0.3, 0.0, 0.3, 0.0, 0.0, 0.6, 0.3, 0.0, 0.3, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, -0.2, 0.2, 0.2, 0.0, 0.4, 0.4, 0.2, 0.2, 0.2, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, -0.1, 0.2, 0.1, 0.0, 0.4, 0.2, 0.1, 0.2, 0.1, 0.0, 0.0, 0.0],
        np.float32).reshape(5, 5, 3)
    normal_ref = np.array([
        0.0, 0.0, 0.0, 0.57735, 0.57735, 0.57735, -0.894427, 0.447214, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, 0.801784, 0.534522, -0.267261, -0.801784, 0.267261, -0.534523, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, 0.57735, -0.57735, -0.57735, -0.666667, -0.333333, -0.666667, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, 0.408248, -0.816497, 0.408248, -0.707107, -0.707107, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
        np.float32).reshape(5, 5, 3)
    clipped = orc.clip_transform(depth, 10.0, 0.0, 2.5, 0.0)
    assert np.allclose(clipped, clipped_ref, rtol=1e-5, atol=1e-8)
    vmap = orc.create_vertex_map(clipped, K, 0.0)
    assert np.allclose(vmap, vertex_ref, rtol=1e-5, atol=1e-8)
    nmap = orc.create_normal_map(vmap, 0.0)
    assert np.allclose(nmap, normal_ref, rtol=1e-5, atol=1e-6)


def test_filter_bilateral_ipp_golden():
    # Image.cpp:246-281 (output_ref_ipp; FilterBilateral(3, 10, 10))
    x = np.zeros((5, 5), np.float32)
    x[2, 2] = 1
    want = np.array([0.0, 0.0, 0.0, 0.0, 0.0,
                     0.0, 0.0, 0.199001, 0.0, 0.0,
                     0.0, 0.199001, 0.201605, 0.199001, 0.0,
                     0.0, 0.0, 0.199001, 0.0, 0.0,
                     0.0, 0.0, 0.0, 0.0, 0.0], np.float32).reshape(5, 5)
    got = orc.filter_bilateral(x, 3, 10, 10)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6)


def test_filter_gaussian_golden():
    # Image.cpp:335-361 (FilterGaussian(3), sigma 1)
    x = np.array([0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                  0, 0, 1, 0], np.float32).reshape(5, 5)
    want = np.array([0.0751136, 0.123841, 0.0751136, 0.0751136, 0.198955,
                     0.123841, 0.204180, 0.123841, 0.123841, 0.328021,
                     0.0751136, 0.123841, 0.0751136, 0.0751136, 0.198955,
                     0.0, 0.0, 0.0751136, 0.123841, 0.0751136,
                     0.0, 0.0, 0.198955, 0.328021, 0.198955],
                    np.float32).reshape(5, 5)
    assert np.allclose(orc.filter_gaussian(x, 3, 1.0), want, rtol=1e-5,
                       atol=1e-7)


def test_filter_sobel_golden():
    # Image.cpp:498-530
    x = np.array([0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0,
                  0, 1, 1, 0], np.float32).reshape(5, 5)
    dx_ref = np.array([1, 1, -1, 2, 3, 2, 3, -2, -2, 1, 0, 3, -1, -4, 0, -2, 2,
                       1, -4, -1, -1, 3, 3, -4, -3], np.float32).reshape(5, 5)
    dy_ref = np.array([1, 3, 3, 0, -3, 0, 1, 2, 0, -3, 2, -1, -1, 0, 0, 0, 0,
                       1, 2, 1, -3, -1, 1, 2, 1], np.float32).reshape(5, 5)
    dx, dy = orc.filter_sobel(x)
    assert np.array_equal(dx, dx_ref)
    assert np.array_equal(dy, dy_ref)


def test_resize_nearest_and_pyrdown_goldens():
    # Image.cpp:565-590 (Resize 0.5 Nearest), :656-681 (PyrDown)
    x = np.array([0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1,
                  0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1],
                 np.float32).reshape(6, 6)
    want = np.array([0, 1, 1, 1, 0, 0, 1, 1, 1], np.float32).reshape(3, 3)
    assert np.array_equal(orc.resize_half_nearest(x), want)
    y = np.array([0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0,
                  0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1],
                 np.float32).reshape(6, 6)
    want = np.array([0.0596343, 0.244201, 0.483257, 0.269109, 0.187536,
                     0.410317, 0.752312, 0.347241, 0.521471],
                    np.float32).reshape(3, 3)
    assert np.allclose(orc.pyrdown(y), want, rtol=1e-5, atol=1e-7)


def test_rgb_to_gray_in_tree_branch():
    # Image.cpp:149-161
    rng = np.random.default_rng(3)
    c8 = rng.integers(0, 256, (16, 20, 3), dtype=np.uint8)
    g = orc.rgb_to_gray(c8)
    f = c8.astype(np.float32)
    want = (f[..., 0] * np.float32(0.299) + f[..., 1] * np.float32(0.587)) \
        + f[..., 2] * np.float32(0.114)
    want = np.clip(np.floor(want.astype(np.float64) + 0.5), 0, 255)
    assert np.array_equal(g, want.astype(np.uint8))
    cf = rng.random((16, 20, 3), dtype=np.float32)
    gf = orc.rgb_to_gray(cf)
    want = (cf[..., 0] * np.float32(0.299) + cf[..., 1] * np.float32(0.587)) \
        + cf[..., 2] * np.float32(0.114)
    assert same_bits(gf, want.astype(np.float32))


# ---------------------------------------------------------------------------
# 2. bit for bit against the reference's own bodies
# ---------------------------------------------------------------------------
def _pair(w=160, h=120, k0=3, step=2, noise=0.0):
    d, c, K, Ts = synthetic.render_frames(k0, 1, w, h, noise_sigma=noise)
    d2, c2, _, Ts2 = synthetic.render_frames(k0 + step, 1, w, h,
                                             noise_sigma=noise, seed=1)
    return (d[0].numpy(), c[0].numpy(), d2[0].numpy(), c2[0].numpy(), K,
            Ts[0], Ts2[0])


def _holes(d, seed=0, frac=0.03):
    rng = np.random.default_rng(seed)
    d = d.copy()
    m = rng.random(d.shape) < frac
    d[m] = 0
    d[10:20, 30:50] = 0
    return d


@needs_ref
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_image_ops_vs_reference_bodies(dtype):
    sd, _, _, _, K, _, _ = _pair(noise=0.002)
    sd = _holes(sd)
    src = sd if dtype == np.uint16 else sd.astype(np.float32)
    for fill in (NAN, 0.0, float("inf")):
        a = orc.clip_transform(src, 1000.0, 0.0, 3.0, fill)
        b = ref.clip_transform(src, 1000.0, 0.0, 3.0, fill)
        assert same_bits(a, b)
        for diff in (0.14, 0.02):
            assert same_bits(orc.pyrdown_depth(a, diff, fill),
                             ref.pyrdown_depth(a, diff, fill))
        va, vb = orc.create_vertex_map(a, K, fill), \
            ref.create_vertex_map(a, K, fill)
        assert same_bits(va, vb)
        assert same_bits(orc.create_normal_map(va, fill),
                         ref.create_normal_map(vb, fill))
    # odd sizes
    odd = orc.clip_transform(src[:119, :157], 1000.0, 0.0, 3.0, NAN)
    assert same_bits(orc.pyrdown_depth(odd, 0.14, NAN),
                     ref.pyrdown_depth(odd, 0.14, NAN))


@needs_ref
def test_image_to_float_vs_reference_body():
    rng = np.random.default_rng(0)
    for arr, scale in ((rng.integers(0, 256, 1000, dtype=np.uint8), 1 / 255),
                       (rng.integers(0, 65536, 1000, dtype=np.uint16),
                        1 / 65535),
                       (rng.standard_normal(1000).astype(np.float32), 2.5)):
        assert same_bits(orc.image_to_float(arr, scale, 0.25),
                         ref.image_to_float(arr, scale, 0.25))


def _levels(noise=0.002):
    """Odometry inputs of one level, built with the oracle's image ops."""
    sd, sc, td, tc, K, Ts, Tt = _pair(noise=noise)
    sd, td = _holes(sd, 1), _holes(td, 2)
    s = orc.clip_transform(sd, 1000.0, 0.0, 3.0, NAN)
    t = orc.clip_transform(td, 1000.0, 0.0, 3.0, NAN)
    sv = orc.create_vertex_map(s, K, NAN)
    tv = orc.create_vertex_map(t, K, NAN)
    tn = orc.create_normal_map(
        orc.create_vertex_map(orc.filter_bilateral(t, 5, 5, 10), K, NAN), NAN)
    si = orc.image_to_float(orc.rgb_to_gray(sc), 1 / 255)
    ti = orc.image_to_float(orc.rgb_to_gray(tc), 1 / 255)
    tdx, tdy = orc.filter_sobel(t)
    tix, tiy = orc.filter_sobel(ti)
    # source -> target of the synthetic trajectory, perturbed so that the
    # residuals are not tiny
    T = Tt @ np.linalg.inv(Ts)
    T = T.copy()
    T[0, 3] += 0.004
    T[2, 3] -= 0.003
    return dict(K=K, T=T, source_vertex=sv, target_vertex=tv, target_normal=tn,
                source_depth=s, target_depth=t, source_intensity=si,
                target_intensity=ti, target_depth_dx=tdx, target_depth_dy=tdy,
                target_intensity_dx=tix, target_intensity_dy=tiy)


@needs_ref
@pytest.mark.parametrize("method", [orc.ODO_P2PLANE, orc.ODO_INTENSITY,
                                    orc.ODO_HYBRID])
@pytest.mark.parametrize("huber", [(0.05, 0.1), (0.004, 0.02)])
def test_odometry_sums_vs_reference_bodies(method, huber):
    L = _levels()
    kw = dict(depth_outlier_trunc=0.07, depth_huber_delta=huber[0],
              intensity_huber_delta=huber[1])
    want_delta, want_res, want_cnt, want_sums = ref.odometry(method, **L, **kw)
    got = orc.odometry_sums(method, **L, **kw, accumulate_double=False)
    assert want_cnt > 1000
    assert np.array_equal(got.astype(np.float32), want_sums.astype(np.float32))
    st, pose, res, cnt = orc.decode_and_solve6x6(got)
    assert st == 0
    assert cnt == want_cnt and np.float32(res) == np.float32(want_res)
    assert np.array_equal(pose, want_delta)
    # float64 accumulators: same terms, so the counts agree exactly and the
    # sums agree to float32 accumulation error
    dbl = orc.odometry_sums(method, **L, **kw, accumulate_double=True)
    assert dbl[28] == got[28]
    assert np.allclose(dbl, got, rtol=2e-3, atol=1e-3)


@needs_ref
def test_odometry_information_vs_reference_body():
    L = _levels()
    want = ref.odometry_information(L["source_vertex"], L["target_vertex"],
                                    L["K"], L["T"], 0.07 * 0.07)
    got = orc.odometry_information(L["source_vertex"], L["target_vertex"],
                                   L["K"], L["T"], 0.07 * 0.07)
    assert np.array_equal(got, want)
    assert got[3, 3] > 1000


# ---------------------------------------------------------------------------
# 3. the multi-scale driver recovers the synthetic relative pose
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", [orc.ODO_P2PLANE, orc.ODO_INTENSITY,
                                    orc.ODO_HYBRID])
def test_multiscale_driver_converges(method):
    sd, sc, td, tc, K, Ts, Tt = _pair(w=320, h=240, step=1)
    r = orc.rgbd_odometry_multiscale(method, sd, td, K, src_color=sc,
                                     tgt_color=tc, accumulate_double=True)
    assert r["status"] == 0
    want = Tt @ np.linalg.inv(Ts)  # source camera -> target camera
    err0 = np.abs(np.eye(4) - want).max()
    err = np.abs(r["transformation"] - want).max()
    assert r["fitness"] > 0.5
    # the photometric term is weak on the procedural (view-shaded) texture
    assert err < (0.35 if method == orc.ODO_P2PLANE else 0.6) * err0, \
        (err, err0)
    f = orc.rgbd_odometry_multiscale(method, sd, td, K, src_color=sc,
                                     tgt_color=tc, accumulate_double=False)
    assert np.abs(f["transformation"] - r["transformation"]).max() < 1e-3


# ---------------------------------------------------------------------------
# 4. crafted one-level inputs (_odometry_cases.py): each regime provably
#    reaches its branch in the oracle, and the oracle equals the reference
#    bodies there
# ---------------------------------------------------------------------------
METHODS = (orc.ODO_P2PLANE, orc.ODO_INTENSITY, orc.ODO_HYBRID)


def _sums(case, method):
    return orc.odometry_sums(method, **case["L"], **case["kw"],
                             accumulate_double=True)


def _info(case):
    L = case["L"]
    return orc.odometry_information(L["source_vertex"], L["target_vertex"],
                                    L["K"], L["T"], case["info_thr"],
                                    accumulate_double=True)


def _result(case, what):
    """29 sums of method `what`, or the information matrix for "info"."""
    return _info(case).ravel() if what == "info" else _sums(case, what)


def _count(case, what):
    return _info(case)[3, 3] if what == "info" else _sums(case, what)[28]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("delta", [0.75, 1.25])
def test_regime_huber_zones(delta, method):
    """Each zone by its signature in J^T r (A[21:27]), which a residual in
    another zone cannot have. Middle zone: derivative 0, so the pixels add
    what no pixel adds and their value does not matter. Tail: +-delta, so the
    value does not matter either, but its being there does. The hybrid method
    sees the values through its 0.707f scale."""
    kw = dict(delta=delta,
              scale=1 / 0.707 if method == orc.ODO_HYBRID else 1.0)
    full = cases.huber_zones(**kw)
    A = _sums(full, method)
    assert A[28] == cases.ROWS * cases.COLS      # nothing is truncated
    b = A[21:27]

    def moved(**change):
        B = _sums(cases.huber_zones(**kw, **change), method)
        assert B[28] == A[28]
        return B[21:27]
    no_mid = _sums(cases.huber_zones(**kw, drop=("mid",)), method)
    assert A[28] - no_mid[28] == full["n_zone"]["mid"] > 0
    # the depth delta rules methods 0 and 2, the intensity delta (0.5) method 1
    mid_is_flat = delta == 0.75 or method == orc.ODO_INTENSITY
    if method == orc.ODO_HYBRID and delta == 1.25:
        # r_I is in its middle zone, r_D in the quadratic one: not flat
        mid_is_flat = False
    if mid_is_flat:
        assert np.array_equal(b, no_mid[21:27])
        assert np.array_equal(b, moved(mid=0.9375, imid=0.9375))
        assert np.any(b != moved(mid=0.375, imid=0.375))    # small zone
    else:       # delta 1.25 swallows the middle zone: derivative r
        assert np.any(b != no_mid[21:27])
        assert np.any(b != moved(mid=0.9375, imid=0.9375))
    no_tail = _sums(cases.huber_zones(**kw, drop=("tail",)), method)
    assert A[28] - no_tail[28] == full["n_zone"]["tail"] > 0
    assert np.any(b != no_tail[21:27])
    assert np.array_equal(b, moved(tail=1.75, itail=1.75))
    assert np.any(b != moved(tail=0.875, itail=0.75))       # middle zone


@pytest.mark.parametrize("method", METHODS)
def test_regime_thresholds(method):
    A = _sums(cases.thresholds(), method)
    B = _sums(cases.thresholds(at_trunc=False), method)
    # 2 of 10 column patterns sit at |r| == trunc: 8 columns x 6 rows
    assert A[28] - B[28] == 8 * cases.ROWS, (A[28], B[28])
    # |r| == delta is in the tail, where Sign(int(0.25)) = 0: those columns
    # are inliers that add nothing to J^T r; 2^-10 below delta they do
    D = _sums(cases.thresholds(
        drop_columns=cases.THRESHOLD_DELTA_COLUMNS[method]), method)
    assert A[28] - D[28] == 8 * cases.ROWS
    assert np.array_equal(A[21:27], D[21:27])
    C = _sums(cases.thresholds(at_delta=False), method)
    assert C[28] == A[28]
    assert np.any(A[21:27] != C[21:27])


def test_regime_behind_camera():
    on = cases.behind_camera()
    for what in METHODS + ("info",):
        n = _count(on, what)
        assert 0 < n < _count(cases.behind_camera(neg=False), what), what
        assert n < _count(cases.behind_camera(zero=False), what), what


def test_regime_boundary():
    on, all_in, all_out = (cases.boundary(m) for m in
                           ("on", "all_in", "all_out"))
    assert on["n_out"] >= 6 and on["n_in"] >= 13
    for what in METHODS + ("info",):
        n = _count(on, what)
        assert _count(all_in, what) - n == on["n_out"], what
        assert n - _count(all_out, what) == on["n_in"], what


@pytest.mark.parametrize("which", cases.NAN_MAPS)
def test_regime_nan_planted(which):
    on, off = cases.nan_planted(which), cases.nan_planted(None)
    for what in METHODS + ("info",):
        a, b = _result(on, what), _result(off, what)
        if what in cases.NAN_AFFECTS[which]:
            assert _count(off, what) - _count(on, what) == \
                len(cases.NAN_PIXELS), (which, what)
            assert np.all(np.isfinite(a))
        else:
            assert np.array_equal(a, b), (which, what)


def test_regime_rotated():
    on, off = cases.rotated(True), cases.rotated(False)
    for what in METHODS + ("info",):
        a, b = _result(on, what), _result(off, what)
        assert _count(on, what) > 1000 and _count(off, what) > 1000
        assert np.all(np.isfinite(a)) and not np.array_equal(a, b)


@needs_ref
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", cases.CRAFTED_NAMES)
def test_crafted_sums_vs_reference_bodies(name, method):
    case = cases.crafted_case(name)
    L, kw = case["L"], case["kw"]
    want_delta, want_res, want_cnt, want_sums = ref.odometry(method, **L, **kw)
    got = orc.odometry_sums(method, **L, **kw, accumulate_double=False)
    assert want_cnt > 0
    assert np.array_equal(got.astype(np.float32), want_sums.astype(np.float32))
    st, pose, res, cnt = orc.decode_and_solve6x6(got)
    assert st == 0
    assert cnt == want_cnt and np.float32(res) == np.float32(want_res)
    assert np.array_equal(pose, want_delta)
    dbl = orc.odometry_sums(method, **L, **kw, accumulate_double=True)
    assert dbl[28] == got[28]
    assert np.allclose(dbl, got, rtol=2e-3, atol=1e-3)


@needs_ref
@pytest.mark.parametrize("name", cases.CRAFTED_NAMES)
def test_crafted_information_vs_reference_body(name):
    case = cases.crafted_case(name)
    L = case["L"]
    want = ref.odometry_information(L["source_vertex"], L["target_vertex"],
                                    L["K"], L["T"], case["info_thr"])
    got = orc.odometry_information(L["source_vertex"], L["target_vertex"],
                                   L["K"], L["T"], case["info_thr"])
    assert np.array_equal(got, want)
    assert got[3, 3] > 0
