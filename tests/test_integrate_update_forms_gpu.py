"""GPU parity of the frame stream's short per-voxel update (vbg_stream.hip,
IntegrateRoleWide: depth tests folded into the prepared records, no underflow
guard on sdf / sdf_trunc, colour as one fma, no uint16 wrap test) and of the
forms a launch or a work item falls back to when a proof does not hold.

Every case integrates 4 frames, edits the voxel state of some blocks where the
case asks for it (on both sides), then integrates 12 more frames in groups of
1, 4 or 12. The whole grid must equal the CPU oracle's, and the same run in a
child process with O3DMI_EXACT_DIV=1 (IEEE divisions, every per-voxel test).

The cases:
  invalid_depths          zero depths and depths beyond depth_max next to
                          valid ones (the records' -inf), voxels projecting
                          outside the image (the sentinel record)
  colour_above_255        colour states up to 40000 with weights 30000-60000
                          in the same blocks: weight * c is far above 2^24,
                          where fma(weight, c, in) and the separate multiply
                          + add round differently -- the work items holding
                          them must keep the multiply + add
  weight_near_wrap        weights within a group's length of 65535 (the wrap)
  depth_scale_fallback    depth_scale = 2^76: RN(1 / depth_scale) < 2^-75, the
                          host rejects the launch and it runs the IEEE-division
                          form (the same kernel the O3DMI_EXACT_DIV child runs,
                          so here only the oracle comparison says something;
                          no voxel comes within 1e-30 of its depth, so this
                          does not exercise the guard itself -- its bound is
                          tested in test_integrate_host_checks.py)
  rejected_pose           one frame of the main phase has a translation of
                          1e35 (beyond the pose bound) and an all-zero depth
                          (it touches nothing): the host sends its whole
                          launch, the other frames of its group included, to
                          the IEEE-division form"""
import json
import os
import subprocess
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

W, H = 320, 240
N_PRE, N_MAIN = 4, 12
CAPACITY = 8192
GROUPS = (1, 4, 12)
CASES = ("invalid_depths", "colour_above_255", "weight_near_wrap",
         "depth_scale_fallback", "rejected_pose")
REJECTED = N_PRE + 5  # the rejected_pose frame: inside a group of 4 and of 12


def _frames(case):
    """Depths (uint16), colours, K, extrinsics and the depth scale of a case."""
    ds, cs, Ts, K = [], [], [], None
    for k in range(200, 200 + 10 * (N_PRE + N_MAIN), 10):
        d, c, K, T = sc.frames(k, 1, W, H)
        ds.append(d[0].copy()); cs.append(c[0]); Ts.append(T[0])
    scale = sc.DEPTH_SCALE
    if case == "invalid_depths":
        # zero depths, depths beyond depth_max (the records' -inf) next to
        # valid ones; voxels near the image border project outside (sentinel)
        for i, d in enumerate(ds):
            d[:, (7 * i) % W:(7 * i) % W + 40] = 0
            d[(11 * i) % H:(11 * i) % H + 30, :] = 60000
            d[::17, ::13] = 0
    elif case == "depth_scale_fallback":
        # RN(1 / depth_scale) < 2^-75: the launches fall back to IEEE forms
        scale = float(2.0 ** 76)
    elif case == "rejected_pose":
        ds[REJECTED][:] = 0
        T = np.array(Ts[REJECTED], np.float64, copy=True)
        T[0, 3] = 1e35  # |e| beyond integrate_checks.h's bound, still finite
        Ts[REJECTED] = T
    return ds, cs, K, Ts, scale


def _edit_state(case, keys, tsdf, weight, color):
    """The state edit of a case on (block-major) numpy views, in place; the
    blocks are chosen from the sorted keys so that both sides agree."""
    if case not in ("colour_above_255", "weight_near_wrap"):
        return
    rng = np.random.default_rng(5)
    order = np.lexsort(keys.T[::-1])
    pick = order[::3]
    for j, b in enumerate(pick):
        if case == "colour_above_255":
            color[b] = rng.integers(0, 40000, color[b].shape).astype(np.uint16)
            weight[b] = rng.integers(30000, 60000, weight[b].shape).astype(
                    np.uint16)
        else:
            weight[b] = (65535 - rng.integers(0, 14, weight[b].shape)).astype(
                    np.uint16)


def _oracle_run(case):
    ds, cs, K, Ts, scale = _frames(case)
    trunc = sc.VOXEL * sc.TRUNC_MULT
    h = orc.HashMap(CAPACITY)
    r = sc.RES
    tsdf = np.zeros((CAPACITY, r, r, r), np.float32)
    wgt = np.zeros((CAPACITY, r, r, r), np.uint16)
    col = np.zeros((CAPACITY, r, r, r, 3), np.uint16)
    for i in range(N_PRE + N_MAIN):
        if i == N_PRE:
            n = h.size()
            keys = h.key_buffer()[:n].copy()
            buf, _ = h.find(keys)
            t, w, c = tsdf[buf], wgt[buf], col[buf]
            _edit_state(case, keys, t, w, c)
            tsdf[buf], wgt[buf], col[buf] = t, w, c
        keys = orc.depth_touch(ds[i], K, Ts[i], r, sc.VOXEL, trunc, scale,
                               sc.DEPTH_MAX, 4)
        if len(keys) == 0:
            continue  # (rejected_pose: a frame that touches nothing)
        h.activate(keys)
        buf, m = h.find(keys)
        assert m.all()
        orc.integrate(ds[i], cs[i], buf, h.key_buffer(), tsdf, wgt, col, K, K,
                      Ts[i], r, sc.VOXEL, trunc, scale, sc.DEPTH_MAX)
    n = h.size()
    keys = h.key_buffer()[:n].copy()
    buf, _ = h.find(keys)
    return keys, tsdf[buf], wgt[buf], col[buf]


def _gpu_run(case, group):
    from open3d_amd import geometry
    ds, cs, K, Ts, scale = _frames(case)
    g = geometry.VoxelBlockGrid(["tsdf", "weight", "color"],
                                [torch.float32, torch.uint16, torch.uint16],
                                [1, 1, 3], voxel_size=sc.VOXEL,
                                block_resolution=sc.RES, block_count=CAPACITY)
    dt = [torch.from_numpy(d).cuda() for d in ds]
    ct = [torch.from_numpy(c).cuda() for c in cs]

    def integrate(lo, hi):
        g.integrate_frames(dt[lo:hi], ct[lo:hi], K, K, Ts[lo:hi], scale,
                           sc.DEPTH_MAX, sc.TRUNC_MULT,
                           frames_per_launch=group)

    def state():
        hm = g.hashmap()
        idx = hm.active_buf_indices()
        keys = hm.key_tensor().cpu().numpy()[idx.cpu().numpy()]
        return keys, idx

    integrate(0, N_PRE)
    torch.cuda.synchronize()
    keys, idx = state()
    i64 = idx.long()
    # uint16 state edited through an int16 view of the same bytes
    wv = g.attribute("weight").view(torch.int16)
    cv = g.attribute("color").view(torch.int16)
    t = g.attribute("tsdf")[i64].cpu().numpy()[..., 0]
    w = wv[i64].cpu().numpy().view(np.uint16)[..., 0]
    c = cv[i64].cpu().numpy().view(np.uint16)
    _edit_state(case, keys, t, w, c)
    wv[i64] = torch.from_numpy(w.view(np.int16)[..., None]).cuda()
    cv[i64] = torch.from_numpy(c.view(np.int16)).cuda()
    integrate(N_PRE, N_PRE + N_MAIN)
    torch.cuda.synchronize()
    keys, idx = state()
    i64 = idx.long()
    t = g.attribute("tsdf")[i64].cpu().numpy()[..., 0]
    w = g.attribute("weight").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16)[..., 0]
    c = g.attribute("color").view(torch.int16)[i64].cpu().numpy().view(
            np.uint16)
    return keys, t, w, c


def _sorted(run):
    keys, t, w, c = run
    o = np.lexsort(np.asarray(keys).T[::-1])
    return (np.asarray(keys)[o], np.ascontiguousarray(t[o]),
            np.ascontiguousarray(w[o]), np.ascontiguousarray(c[o]))


def _same(a, b):
    for x, y in zip(_sorted(a), _sorted(b)):
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


@pytest.fixture(scope="module")
def exact_div_runs(tmp_path_factory):
    """Every (case, group) once more in ONE child process with the IEEE
    division forms (O3DMI_EXACT_DIV is read once per process)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = str(tmp_path_factory.mktemp("exact") / "runs.npz")
    env = dict(os.environ, O3DMI_EXACT_DIV="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("case", CASES)
def test_update_forms_equal_oracle_and_ieee_forms(case, group,
                                                  exact_div_runs):
    got = _gpu_run(case, group)
    want = _oracle_run(case)
    ks, ts, ws, cs = _sorted(got)
    kw, tw, ww, cw = _sorted(want)
    assert np.array_equal(ks, kw)
    assert np.array_equal(ws, ww)
    assert np.array_equal(cs, cw)
    assert ts.tobytes() == tw.tobytes()
    if case == "weight_near_wrap":
        assert (ws < 100).any() and (ws > 65500).any()  # wrapped and not
    if case == "colour_above_255":
        assert (cs > 255).any() and (ws > 30000).any()
    ieee = tuple(exact_div_runs["%s_%d_%d" % (case, group, i)]
                 for i in range(4))
    assert _same(got, ieee)


def _child(out):
    torch.cuda.set_device(0)
    runs = {}
    for case in CASES:
        for group in GROUPS:
            for i, a in enumerate(_gpu_run(case, group)):
                runs["%s_%d_%d" % (case, group, i)] = np.asarray(a)
    np.savez(out, **runs)
    print(json.dumps({"runs": len(runs)}))


if __name__ == "__main__":
    _child(sys.argv[1])
