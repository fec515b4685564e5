# How often the two voxels of every lane of an integrate wave share their
# weight arithmetic (CPU estimate on the bench stream).
#
# A lane of the integrate role owns two x-adjacent voxels; with `cube` on, a
# wave covers a (4 pairs x 4 x 4) cube of a 16^3 block. If in EVERY lane the
# two voxels enter a frame with the same weight and take the same update
# predicate, then w + 1, 1 / (w + 1) and the new weight are the same float for
# both and one copy is redundant. This replays every 10th frame of the
# 1000-frame stream with the CPU oracle, twice (the second pass starts from
# history-shaped weights), and reports, among the (wave cube, frame) pairs
# that update at least one voxel, the share P where both conditions hold.
#
#   python tools/pair_weight_estimate.py > profiles/r11_pair_weight_estimate.txt
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from open3d_amd import synthetic as syn  # noqa: E402
import _oracle as orc  # noqa: E402

W, H = 640, 480
VOX = 0.008; RES = 16; TRUNC = 8 * VOX; DS = 1000.0; DMAX = 3.0
CAP = 16384
K = syn.intrinsics(W, H)


def cubes(a):
    """(n, 16, 16, 16) [z, y, x] -> (n * 32 waves, 64 lanes, 2 voxels): the
    role's lane map, q = qx_lo | y_lo << 2 | z_lo << 4 | wave << 6."""
    n = a.shape[0]
    a = a.reshape(n, 4, 4, 4, 4, 2, 4, 2)  # z_hi z_lo y_hi y_lo x_hi pair h
    a = a.transpose(0, 1, 3, 5, 2, 4, 6, 7)
    return a.reshape(n * 32, 64, 2)


frames = []
for k in range(0, 1000, 10):
    d, c, _, T = syn.render_frames(k, 1, W, H, device="cpu")
    frames.append((d[0].numpy(), c[0].numpy(), np.asarray(T[0], np.float64)))

h = orc.HashMap(CAP)
tsdf = np.zeros((CAP, RES, RES, RES), np.float32)
wgt = np.zeros((CAP, RES, RES, RES), np.uint16)
col = np.zeros((CAP, RES, RES, RES, 3), np.uint16)
print("pair-weight fact, bench stream, every 10th frame, %d x %d, res %d, "
      "wave cube 4 pairs x 4 x 4" % (W, H, RES))
for p in range(2):
    live = both = entry = pred = 0
    for d, c, T in frames:
        keys = orc.depth_touch(d, K, T, RES, VOX, TRUNC, DS, DMAX, 4)
        h.activate(keys)
        buf, m = h.find(keys)
        assert m.all()
        before = wgt[buf].copy()
        orc.integrate(d, c, buf, h.key_buffer(), tsdf, wgt, col, K, K, T, RES,
                      VOX, TRUNC, DS, DMAX)
        wb = cubes(before)
        up = cubes(wgt[buf] != before)  # the update moves the weight by + 1
        is_live = up.any(axis=(1, 2))
        e = (wb[..., 0] == wb[..., 1]).all(axis=1)
        q = (up[..., 0] == up[..., 1]).all(axis=1)
        live += int(is_live.sum())
        entry += int((is_live & e).sum())
        pred += int((is_live & q).sum())
        both += int((is_live & e & q).sum())
    print("pass %d: (wave cube, frame) pairs updating a voxel %d; weights equal "
          "on entry %.4f; predicates equal %.4f; P (both) %.4f; priced saving "
          "P x 17.9 / 350 = %.2f %%"
          % (p + 1, live, entry / live, pred / live, both / live,
             100 * both / live * 17.9 / 350))
print("blocks in the map", h.size(), "max weight", int(wgt.max()))
