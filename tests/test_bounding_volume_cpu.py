"""CPU checks of the oriented bounding boxes and the bounding ellipsoid: the
numpy oracle (tests/_bounding_volume_oracle.py) against closed forms, the two
host-only functions of the library through ctypes against numpy.linalg.eigh,
and the places where the rules are written down. No GPU."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import _bounding_volume_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)


# ---- the clouds the GPU tests share -------------------------------------------------
def random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def box_cloud():
    """The 8 corners of a 2 x 4 x 6 box and 200 interior points under a random
    rotation and offset -> (points, rotation, offset)."""
    rng = np.random.default_rng(1)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-2, 2)
                        for z in (-3, 3)], np.float64)
    inner = (rng.random((200, 3)) - 0.5) * np.array([2.0, 4.0, 6.0]) * 0.98
    q = random_rotation(rng)
    offset = np.array([5.0, -3.0, 2.0])
    return np.concatenate([corners, inner]) @ q.T + offset, q, offset


def gaussian_cloud(dtype=np.float64):
    """300 points, sigma = (3, 2, 1)."""
    rng = np.random.default_rng(2)
    g = rng.standard_normal((300, 3)) * np.array([3.0, 2.0, 1.0])
    return g.astype(dtype)


def scaled_sphere(n, seed=5, dtype=np.float64):
    """n points on the ellipsoid with semi-axes (3, 2, 1), turned out of the
    coordinate axes: every point is a hull vertex."""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    g = g / np.linalg.norm(g, axis=1, keepdims=True)
    q = random_rotation(np.random.default_rng(7))
    return ((g * np.array([3.0, 2.0, 1.0])) @ q.T).astype(dtype)


@functools.lru_cache(maxsize=None)
def gaussian_hull():
    return orc.hull_of(gaussian_cloud())


@functools.lru_cache(maxsize=None)
def box_hull():
    return orc.hull_of(box_cloud()[0])


def inside_box(points, center, R, extent, slack):
    c = (np.asarray(points, np.float64) - center) @ R
    return bool((np.abs(c) <= extent / 2.0 + slack).all())


def inside_ellipsoid(points, center, Q, max_m, slack):
    """(x - c)^T Q (x - c) <= (max M - 1) / 3 + slack. With Q made of the
    weights p, (x - c)^T Q (x - c) = (M_i - 1) / 3 exactly, M evaluated at the
    SAME p. The loop's last iteration evaluates M before its weight update and
    Q is made of the weights after it, so max_m must be the oracle's
    final_max_m; the last iteration's maximum bounds nothing (on the Gaussian
    cloud the largest left side is 4.8e-4 above it)."""
    d = np.asarray(points, np.float64) - center
    v = np.einsum("ni,ij,nj->n", d, Q, d)
    return bool((v <= (max_m - 1.0) / 3.0 + slack).all())


# ---- the oracle against closed forms ------------------------------------------------
def test_tree_sum_is_the_sum():
    rng = np.random.default_rng(3)
    for n in (1, 7, 8, 9, 64, 65, 513, 4097):
        v = rng.standard_normal((n, 2))
        t = orc.tree_sum(v)
        assert np.allclose(t, v.sum(axis=0), rtol=0, atol=1e-12 * n)
        assert np.array_equal(orc.tree_sum(v[:, 0]), t[0])
    # written out: ((0 + a) + b) for one short run
    assert orc.tree_sum(np.array([0.1, 0.2, 0.3])) == ((0.0 + 0.1) + 0.2) + 0.3
    v = rng.standard_normal(20)
    runs = [functools.reduce(lambda a, b: a + b, v[k:k + 8], 0.0)
            for k in (0, 8, 16)]
    assert orc.tree_sum(v) == ((0.0 + runs[0]) + runs[1]) + runs[2]


def test_box_cloud_minimal_approx_is_the_box():
    points, q, offset = box_cloud()
    X, tri, _ = box_hull()
    assert len(X) == 8 and len(tri) == 12
    r = orc.minimal_approx(X, tri)
    e = r["extent"]
    assert abs((e[0] * e[1]) * e[2] - 48.0) <= 1e-12 * 48.0
    diagonal = float(np.linalg.norm([2.0, 4.0, 6.0]))
    got = orc.box_points(r["center"], r["rotation"], e)
    want = points[:8]
    d = np.linalg.norm(got[:, None, :] - want[None, :, :], axis=2)
    assert (d.min(axis=1) <= 1e-12 * diagonal).all()
    assert sorted(d.argmin(axis=1)) == list(range(8))


def test_box_cloud_ellipsoid_stops_after_one_iteration():
    points, q, offset = box_cloud()
    X, tri, _ = box_hull()
    r = orc.ellipsoid(X)
    assert r["iterations"] == 1
    assert np.allclose(r["center"], offset, rtol=0, atol=1e-12)
    want = np.sqrt(3.0) * np.array([1.0, 2.0, 3.0])
    assert np.allclose(np.sort(r["radii"]), want, rtol=1e-12, atol=0)


def test_gaussian_cloud_pca_diagonalises_the_covariance():
    X, tri, _ = gaussian_hull()
    r = orc.pca(X)
    R = r["rotation"]
    cov = np.cov(X.T, bias=True)
    D = R.T @ cov @ R
    off = D - np.diag(np.diag(D))
    assert np.abs(off).max() <= 1e-12 * np.abs(cov).max()
    assert D[0, 0] >= D[1, 1] >= D[2, 2]
    assert np.allclose(R.T @ R, np.eye(3), rtol=0, atol=1e-12)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12


def test_gaussian_cloud_lies_inside_all_three_volumes():
    points = gaussian_cloud()
    X, tri, _ = gaussian_hull()
    s = orc.slack(points)
    for r in (orc.minimal_approx(X, tri), orc.pca(X)):
        assert inside_box(points, r["center"], r["rotation"], r["extent"], s)
    e = orc.ellipsoid(X)
    assert e["iterations"] == orc.MAX_ITERATIONS
    assert inside_ellipsoid(points, e["center"], e["Q"], e["final_max_m"], s)
    assert abs(e["max_m"] - 4.011) < 1e-3  # the loop ran out of iterations
    # the winner is unique by a wide margin (the GPU test compares bits)
    v = np.sort(orc.minimal_approx(X, tri)["volumes"])
    assert v[1] >= v[0] * (1.0 + 1e-6)


# ---- the host-only functions --------------------------------------------------------
@pytest.fixture(scope="module")
def so():
    import __graft_entry__ as ge
    ge.build()
    from open3d_amd import _lib
    L = C.CDLL(_lib.SO_PATH)
    L.o3dmi_bounding_box_frame_from_moments.argtypes = [C.c_int64, _dp, _dp,
                                                        _dp]
    L.o3dmi_bounding_ellipsoid_from_moments.argtypes = [_dp, _dp, _dp, _dp]
    return L


def _f64(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(_dp)


def frame_from_moments(so, n, sums):
    sums, ps = _f64(sums)
    mean, pm = _f64(np.full(3, -777.0))
    R, pr = _f64(np.full(9, -777.0))
    st = so.o3dmi_bounding_box_frame_from_moments(n, ps, pm, pr)
    return st, mean, R.reshape(3, 3)


def ellipsoid_from_moments(so, sums):
    sums, ps = _f64(sums)
    c, pc = _f64(np.full(3, -777.0))
    R, pr = _f64(np.full(9, -777.0))
    radii, pd = _f64(np.full(3, -777.0))
    st = so.o3dmi_bounding_ellipsoid_from_moments(ps, pc, pr, pd)
    return st, c, R.reshape(3, 3), radii


def spd_matrices():
    """100 random symmetric positive definite matrices with eigenvalue ratios
    >= 2 -> (matrix, eigenvalues descending, mean)."""
    rng = np.random.default_rng(11)
    out = []
    for _ in range(100):
        small = 10.0 ** rng.uniform(-3, 3)
        lam = small * np.cumprod([1.0, rng.uniform(2, 10), rng.uniform(2, 10)])
        q = random_rotation(rng)
        out.append((q @ np.diag(lam) @ q.T, lam[::-1].copy(),
                    rng.standard_normal(3) * np.sqrt(small)))
    return out


def sums_of(cov, mean, n):
    """The nine sums of n points with this mean and covariance."""
    second = cov + np.outer(mean, mean)
    return n * np.array([mean[0], mean[1], mean[2], second[0, 0], second[0, 1],
                         second[0, 2], second[1, 1], second[1, 2],
                         second[2, 2]])


def test_frame_from_moments_against_eigh(so):
    for cov, lam, mean in spd_matrices():
        n = 1000
        sums = sums_of(cov, mean, n)
        st, got_mean, R = frame_from_moments(so, n, sums)
        assert st == 0
        assert np.array_equal(got_mean, sums[:3] / n)
        # the covariance the function itself forms (its cancellation is the
        # input's, not Jacobi's)
        c = sums / n
        C_ = np.array([[c[3] - c[0] * c[0], c[4] - c[0] * c[1],
                        c[5] - c[0] * c[2]],
                       [c[4] - c[0] * c[1], c[6] - c[1] * c[1],
                        c[7] - c[1] * c[2]],
                       [c[5] - c[0] * c[2], c[7] - c[1] * c[2],
                        c[8] - c[2] * c[2]]])
        w = np.linalg.eigh(C_)[0][::-1]
        norm = np.linalg.norm(C_, 2)
        for k in range(3):
            assert np.linalg.norm(C_ @ R[:, k] - w[k] * R[:, k]) <= \
                1e-12 * norm
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
        assert abs(np.linalg.det(R) - 1.0) <= 1e-12
        for k in range(2):  # the sign rule
            big = int(np.argmax(np.abs(R[:, k])))
            assert R[big, k] > 0
        # and the oracle states the same function, bit for bit
        o_mean, o_R = orc.frame_from_moments(n, sums)
        assert np.array_equal(o_R, R) and np.array_equal(o_mean, got_mean)


def test_ellipsoid_from_moments_against_eigh(so):
    for cov, lam, mean in spd_matrices():
        sums = sums_of(cov, mean, 1)
        st, c, R, radii = ellipsoid_from_moments(so, sums)
        assert st == 0
        assert np.array_equal(c, sums[:3])
        S = np.array([[sums[3] - c[0] * c[0], sums[4] - c[0] * c[1],
                       sums[5] - c[0] * c[2]],
                      [sums[4] - c[0] * c[1], sums[6] - c[1] * c[1],
                       sums[7] - c[1] * c[2]],
                      [sums[5] - c[0] * c[2], sums[7] - c[1] * c[2],
                       sums[8] - c[2] * c[2]]])
        Q = np.linalg.inv(S) / 3.0
        norm = np.linalg.norm(Q, 2)
        for k in range(3):
            lam_k = 1.0 / (radii[k] * radii[k])
            # the inverse of S costs cond(S) <= 100 roundings, Jacobi none
            assert np.linalg.norm(Q @ R[:, k] - lam_k * R[:, k]) <= \
                1e-12 * norm
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
        assert np.allclose(np.sort(radii), np.sqrt(3.0 * np.sort(
            np.linalg.eigvalsh(S))), rtol=1e-12, atol=0)
        o_c, o_R, o_radii, _ = orc.ellipsoid_from_moments(sums)
        assert np.array_equal(o_R, R) and np.array_equal(o_radii, radii)


def test_closest_identity_on_all_48_signed_permutations(so):
    """Whatever signed permutation of a known frame's axes the moments hide,
    the canonical frame comes back: the moments do not see it, and the
    oracle's closest_identity, fed each of the 48, returns the frame itself."""
    rng = np.random.default_rng(12)
    # a frame close to the identity: it is its own closest candidate
    w = rng.standard_normal(3) * 0.2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    F = np.linalg.qr(np.eye(3) + K)[0]
    F = F * np.sign(np.diag(F))[None, :]
    radii = np.array([1.5, 0.7, 2.5])
    seen = 0
    for p in itertools.permutations(range(3)):
        for signs in itertools.product((-1.0, 1.0), repeat=3):
            V = F[:, list(p)] * np.array(signs)[None, :]
            R, r = orc.closest_identity(V.tolist(), radii[list(p)].tolist())
            assert np.array_equal(R, F) and np.array_equal(r, radii)
            seen += 1
    assert seen == 48
    # through the library: the ellipsoid with these axes and radii
    S = F @ np.diag(radii * radii / 3.0) @ F.T
    st, c, R, got = ellipsoid_from_moments(so, sums_of(S, np.zeros(3), 1))
    assert st == 0
    assert np.allclose(R, F, rtol=0, atol=1e-12)
    assert np.allclose(got, radii, rtol=1e-12, atol=0)


def test_host_functions_refuse_and_leave_outputs(so):
    good = sums_of(np.eye(3), np.zeros(3), 10)
    bad = good.copy()
    bad[4] = np.nan
    for st, *outs in (frame_from_moments(so, 0, good),
                      frame_from_moments(so, 10, bad),
                      ellipsoid_from_moments(so, bad)):
        assert st == 1
        assert all((o == -777.0).all() for o in outs)
    flat = sums_of(np.diag([1.0, 1.0, 0.0]), np.zeros(3), 1)
    st, *outs = ellipsoid_from_moments(so, flat)
    assert st == 5 and all((o == -777.0).all() for o in outs)
    assert so.o3dmi_bounding_box_frame_from_moments(10, None, None, None) == 1
    assert so.o3dmi_bounding_ellipsoid_from_moments(None, None, None,
                                                    None) == 1


# ---- where the rules are written down -----------------------------------------------
def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_abi_listing_and_constants():
    from open3d_amd import _lib
    host_h = _read("include", "o3d_mi355x_host.h")
    seam = _read("open3d_amd", "csrc", "bounding_volume.h")
    for name in ("o3dmi_pointcloud_oriented_bounding_box",
                 "o3dmi_pointcloud_oriented_bounding_ellipsoid",
                 "o3dmi_bounding_box_frame_from_moments",
                 "o3dmi_bounding_ellipsoid_from_moments"):
        assert name + "(" in host_h and name in _lib.PROTOTYPES, name
    for name in ("o3dmi_internal_pointcloud_obb_minimal_approx",
                 "o3dmi_internal_obe_resident_capacity",
                 "o3dmi_internal_bounding_volume_stats"):
        assert name in seam and name in _lib.INTERNAL_PROTOTYPES, name
    run = int(re.search(r"constexpr int kBvRun = (\d+);", seam).group(1))
    assert run == orc.RUN
    assert "#define O3DMI_BV_TREE_RUN %d\n" % run in host_h
    assert "constexpr double kObeTolerance = 1e-6;" in seam
    assert "constexpr int kObeMaxIterations = 1000;" in seam
    assert "#define O3DMI_OBE_TOLERANCE 1e-6\n" in host_h
    assert "#define O3DMI_OBE_MAX_ITERATIONS 1000\n" in host_h
    assert (orc.TOLERANCE, orc.MAX_ITERATIONS) == (1e-6, 1000)
    assert "#define O3DMI_OBB_MINIMAL_APPROX 0" in host_h
    assert "#define O3DMI_OBB_PCA 1" in host_h
    assert "#define O3DMI_OBB_MINIMAL_JYLANKI 2" in host_h
    sweeps = int(re.search(r"constexpr int kJacobiSweeps = (\d+);", _read(
        "open3d_amd", "csrc", "eigen3.h")).group(1))
    assert sweeps == orc.JACOBI_SWEEPS
    for rule in ("std::random_device", "strict <", "O3DMI_ERR_SINGULAR",
                 "O3DMI_ERR_UNSUPPORTED", "n >= 2^31 - 1", "untouched",
                 "the transpose is the same", "cast to Float32",
                 "lowest index on ties", "O3DMI_ERR_CAPACITY"):
        assert rule in host_h, rule
    # the hull is handed over through one declaration
    hull_host = _read("open3d_amd", "csrc", "host", "pointcloud_hull_host.h")
    assert "struct HullOutput" in hull_host and "int HullOf(" in hull_host
    for driver in ("pointcloud_hull.cpp", "bounding_volume.cpp"):
        text = _read("open3d_amd", "csrc", "host", driver)
        assert '#include "pointcloud_hull_host.h"' in text
        assert "struct HullOutput" not in text


def test_switches_and_docs_are_listed():
    switches = _read("docs", "switches.md")
    driver = _read("open3d_amd", "csrc", "host", "bounding_volume.cpp")
    assert "`O3DMI_OBE_FORM`" in switches and "O3DMI_OBE_FORM" in driver
    assert "kObeBatch" in driver
    doc = _read("docs", "bounding_volumes.md")
    for word in ("kBvRun", "kObeResidentCapacity", "MINIMAL_JYLANKI",
                 "transpose", "Float32", "kObeBatch", "kObbMaxSplit",
                 "64 times"):
        assert word in doc, word
    readme = _read("README.md")
    assert "bounding_volume.hip" in readme
    assert "host/bounding_volume.cpp" in readme
    assert "docs/bounding_volumes.md" in readme


def test_python_layer_refuses_robust():
    from open3d_amd import pointcloud, trianglemesh
    for call in (pointcloud.get_oriented_bounding_box,
                 pointcloud.get_oriented_bounding_ellipsoid,
                 trianglemesh.get_oriented_bounding_box,
                 trianglemesh.get_oriented_bounding_ellipsoid):
        with pytest.raises(ValueError, match="robust"):
            call({"positions": None}, robust=True)
    with pytest.raises(ValueError, match="method"):
        pointcloud.get_oriented_bounding_box({}, method="obb")
