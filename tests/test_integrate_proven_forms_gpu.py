"""GPU parity of the frame stream's proven form (vbg_stream.hip,
FrameStepKernelProven: no range test of the projection's 1 / z) and of the form
a group falls back to when the proof does not hold for it.

Every case integrates 13 frames of 64 x 48 pixels into an 8 mm grid with
frames_per_launch = 12 -- one full group and one group of a single frame -- at
block resolutions 16 and 8. TSDF, weight and colour must equal the CPU
oracle's bit for bit.

  ordinary        scene poses: both groups run the proven form
  identity_pose   one frame of the full group has the identity extrinsic
                  (e[2][3] = 0, RcpRangePoseOk rejects it): the whole group
                  takes the form with the range test, the 1-frame group after
                  it the proven form
  camera_plane    depths of 2 - 20 cm, so that the camera plane cuts through
                  the touched blocks: lanes with z < 0, z = 0 exactly and z a
                  few float steps above 0 next to updated lanes, all in the
                  proven form (axis-aligned poses whose translation cancels a
                  voxel plane's z, or misses it by a step; oblique scene poses)
  other_colour    a 32 x 24 colour image with its own intrinsics: the prepare
                  pass leaves records without a colour, which the proven form
                  must skip like every other (it keeps the records' colour
                  flag test)
  border_column   depth and colour of one size and intrinsics, but intrinsics
                  (the scene generator's own for 64 x 48, fx = 52.5) whose
                  float32 Unproject -> Project puts column 0 at u = -2e-6,
                  outside the colour image: records without a colour in a
                  same-size pair
  colourless      a grid without colour: proven form"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _oracle as orc  # noqa: E402
import _scene as sc  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
CW, CH = 32, 24
N, GROUP = 13, 12
CAPACITY = 4096
IDENTITY_FRAME = 5
CASES = ("ordinary", "identity_pose", "camera_plane", "other_colour",
         "border_column", "colourless")
# Intrinsics with a power-of-two focal length: (u - cx) / fx * fx + cx is exact,
# so the prepare tables of a depth / colour pair of one size are the identity.
# (The images were rendered with the scene generator's intrinsics; to the
# integration they are just depths and colours.)
K_EXACT = np.array([[64.0, 0, 31.5], [0, 64.0, 23.5], [0, 0, 1]])
KC_SMALL = np.array([[32.0, 0, 15.5], [0, 32.0, 11.5], [0, 0, 1]])
# integrate launches by form (o3dmi_vbg_step_form_launches): IEEE divisions,
# short divisions, proven -- for the 12-frame and the 1-frame group
WANT_FORMS = {
    "ordinary": (0, 0, 2), "identity_pose": (0, 1, 1),
    "camera_plane": (0, 0, 2), "other_colour": (0, 0, 2),
    "border_column": (0, 0, 2), "colourless": (0, 0, 2),
}
F = np.float32
Z_PLANE = 3  # camera_plane: the voxel plane whose z the translation cancels


def _plane_pose(step):
    """Axis-aligned pose with e[2][3] = -(Z_PLANE * voxel) as the kernel rounds
    it, moved by `step` float32 steps: the voxels of that plane get z = 0
    (step 0) or z = one or two steps of the sum above / below 0."""
    t = -(F(Z_PLANE) * F(sc.VOXEL))
    for _ in range(abs(step)):
        t = np.nextafter(t, F(np.inf if step > 0 else -np.inf))
    T = np.eye(4)
    T[2, 3] = float(t)
    return T


@pytest.fixture(scope="module")
def scene():
    ds, cs, cs_small, Ts = [], [], [], []
    K_scene = None
    for k in range(200, 200 + 10 * N, 10):
        d, c, K_scene, T = sc.frames(k, 1, W, H)
        _, c2, _, _ = sc.frames(k, 1, CW, CH)
        ds.append(d[0]); cs.append(c[0]); cs_small.append(c2[0])
        Ts.append(np.array(T[0], np.float64))
    return dict(ds=ds, cs=cs, cs_small=cs_small, Ts=Ts, K_scene=K_scene)


def _inputs(case, scene):
    """depths, colours (or None), K, colour K, extrinsics of a case"""
    ds, cs, Ts = list(scene["ds"]), list(scene["cs"]), list(scene["Ts"])
    K = Kc = K_EXACT
    if case == "identity_pose":
        Ts[IDENTITY_FRAME] = np.eye(4)
    elif case == "camera_plane":
        rng = np.random.default_rng(3)
        ds = [rng.integers(20, 200, (H, W)).astype(np.uint16) for _ in ds]
        for i, step in enumerate((0, 1, -1, 2)):
            Ts[2 * i] = _plane_pose(step)
        Ts[N - 1] = _plane_pose(1)  # the 1-frame group as well
    elif case == "other_colour":
        cs, Kc = list(scene["cs_small"]), KC_SMALL
    elif case == "border_column":
        K = Kc = scene["K_scene"]
    elif case == "colourless":
        cs = None
    return ds, cs, K, Kc, Ts


def _oracle_run(case, res, scene):
    ds, cs, K, Kc, Ts = _inputs(case, scene)
    trunc = sc.VOXEL * sc.TRUNC_MULT
    h = orc.HashMap(CAPACITY)
    tsdf = np.zeros((CAPACITY, res, res, res), np.float32)
    wgt = np.zeros((CAPACITY, res, res, res), np.uint16)
    col = np.zeros((CAPACITY, res, res, res, 3), np.uint16) if cs else None
    for i in range(N):
        keys = orc.depth_touch(ds[i], K, Ts[i], res, sc.VOXEL, trunc,
                               sc.DEPTH_SCALE, sc.DEPTH_MAX, 4)
        assert len(keys) > 0
        h.activate(keys)
        buf, m = h.find(keys)
        assert m.all()
        orc.integrate(ds[i], cs[i] if cs else None, buf, h.key_buffer(), tsdf,
                      wgt, col, K, Kc, Ts[i], res, sc.VOXEL, trunc,
                      sc.DEPTH_SCALE, sc.DEPTH_MAX)
    n = h.size()
    keys = h.key_buffer()[:n].copy()
    buf, _ = h.find(keys)
    return keys, tsdf[buf], wgt[buf], col[buf] if cs else None


def _form_counts(L):
    return tuple(int(L.o3dmi_vbg_step_form_launches(f)) for f in range(3))


def _gpu_run(case, res, scene):
    from open3d_amd import _lib, geometry
    L = _lib.lib()
    # launches take the IEEE forms until the on-device proof of the short
    # divisions is over: wait for it, so that the forms below are determined
    assert L.o3dmi_vbg_division_forms(C.c_float(sc.VOXEL),
                                      C.c_float(sc.TRUNC_MULT), 1) == 2
    ds, cs, K, Kc, Ts = _inputs(case, scene)
    names = ["tsdf", "weight"] + (["color"] if cs else [])
    dtypes = [torch.float32, torch.uint16] + ([torch.uint16] if cs else [])
    g = geometry.VoxelBlockGrid(names, dtypes, [1, 1] + ([3] if cs else []),
                                voxel_size=sc.VOXEL, block_resolution=res,
                                block_count=CAPACITY)
    dt = [torch.from_numpy(d).cuda() for d in ds]
    ct = [torch.from_numpy(c).cuda() for c in cs] if cs else None
    before = _form_counts(L)
    g.integrate_frames(dt, ct, K, Kc, Ts, sc.DEPTH_SCALE, sc.DEPTH_MAX,
                       sc.TRUNC_MULT, frames_per_launch=GROUP)
    torch.cuda.synchronize()
    forms = tuple(a - b for a, b in zip(_form_counts(L), before))
    hm = g.hashmap()
    idx = hm.active_buf_indices()
    keys = hm.key_tensor().cpu().numpy()[idx.cpu().numpy()]
    i64 = idx.long()
    t = g.attribute("tsdf")[i64].cpu().numpy()[..., 0]
    w = g.attribute("weight").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16)[..., 0]
    c = g.attribute("color").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16) if cs else None
    return (keys, t, w, c), forms


def _sorted(run):
    keys, t, w, c = run
    o = np.lexsort(np.asarray(keys).T[::-1])
    return (np.asarray(keys)[o], np.ascontiguousarray(t[o]),
            np.ascontiguousarray(w[o]),
            np.ascontiguousarray(c[o]) if c is not None else None)


@pytest.mark.parametrize("res", [16, 8])
@pytest.mark.parametrize("case", CASES)
def test_proven_form_and_its_fallbacks_equal_the_oracle(case, res, scene):
    got, forms = _gpu_run(case, res, scene)
    ks, ts, ws, cs = _sorted(got)
    kw, tw, ww, cw = _sorted(_oracle_run(case, res, scene))
    assert np.array_equal(ks, kw)
    assert np.array_equal(ws, ww)
    assert ts.tobytes() == tw.tobytes()
    if case == "colourless":
        assert cs is None
    else:
        assert np.array_equal(cs, cw)
        assert (cs > 0).any()
    assert (ws > 0).any() and (ws == 0).any()
    assert forms == WANT_FORMS[case], forms
    if case == "camera_plane":
        # what the case is there for, on the kernel's own float32 sums: in the
        # touched blocks around the camera the axis-aligned frames see voxels
        # behind the camera plane, on it (step 0) and a float step or two
        # above it (steps 1, 2), and voxels of those blocks are updated
        zc = np.unique(ks[:, 2:3] * res + np.arange(res)[None, :])
        zs = zc.astype(F) * F(sc.VOXEL)
        z = {s: zs + F(_plane_pose(s)[2, 3]) for s in (0, 1, 2)}
        assert (z[0] == 0).any() and (z[0] < 0).any() and (z[0] > 0).any()
        for s in (1, 2):
            assert ((z[s] > 0) & (z[s] < F(1e-8))).any()
        near = (ks[:, 2] == 0)  # the blocks the plane z = Z_PLANE voxels is in
        assert near.any() and (ws[near] > 0).any() and (ws[near] == 0).any()
