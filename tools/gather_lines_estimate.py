# How many distinct 128-byte cache lines a record gather of the integrate role
# touches, under two lane -> voxel maps (CPU estimate on the bench stream,
# DESIGN sections 3 and 4).
#
# A wave of the role covers an 8 x 4 x 4 cube of a 16^3 block; a lane owns two
# voxels of it and a frame costs the wave two gather instructions, one per
# voxel slot, 64 records of 8 bytes each out of the frame's record image
# (row-major, pitch cols * 8, one sentinel record behind the last row for
# voxels that project outside the image).
#   (A) today's map: the lane's voxels are x-adjacent, x = 2 j + h (lane field
#       j = 0..3, slot h): an instruction covers x in {h, h+2, h+4, h+6};
#   (B) the lane's voxels are x = j and j + 4: an instruction covers a compact
#       4 x 4 x 4 cube (which lane of a quad takes which j does not change the
#       set of lines).
# This replays every 10th frame of the 1000-frame stream: the blocks of a frame
# come from the oracle's depth touch, the projection is the role's own float32
# sequence (Camera::RigidTransform, Project, InBoundary). Counted per (wave
# cube, frame) pair the role issues gathers for (every wave of a block the
# frame touches), and again for the live ones among them (a voxel updates).
#
#   python tools/gather_lines_estimate.py > profiles/r12_gather_lines.txt
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
REC = 8          # bytes per record
LINE = 128       # bytes per cache line
K = syn.intrinsics(W, H)
f32 = np.float32


def project(keys, T):
    """keys (n, 3) -> line index and in-image flag of every voxel's record,
    (n, 16, 16, 16) [z, y, x], and the camera z: the role's float32 steps."""
    e = np.asarray(T, np.float64)[:3].astype(f32)
    g = np.arange(RES, dtype=np.int64)
    vs = f32(VOX)
    xs = (keys[:, 0, None] * RES + g).astype(f32)[:, None, None, :] * vs
    ys = (keys[:, 1, None] * RES + g).astype(f32)[:, None, :, None] * vs
    zs = (keys[:, 2, None] * RES + g).astype(f32)[:, :, None, None] * vs
    row = lambda i: ((xs * e[i, 0] + ys * e[i, 1]) + zs * e[i, 2]) + e[i, 3]
    xc, yc, zc = row(0), row(1), row(2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_z = f32(1.0) / zc
        u = xc * f32(K[0, 0]) * inv_z + f32(K[0, 2])
        v = yc * f32(K[1, 1]) * inv_z + f32(K[1, 2])
        inb = (u >= 0) & (u <= f32(W - 1)) & (v >= 0) & (v <= f32(H - 1))
    ui = np.where(inb, u, 0).astype(np.int64)
    vi = np.where(inb, v, 0).astype(np.int64)
    off = np.where(inb, vi * (W * REC) + ui * REC, H * W * REC)
    return off // LINE, inb, zc, ui, vi


def waves(a, b_map):
    """(n, 16, 16, 16) [z, y, x] -> (n * 32 waves, 2 slots, 64 lanes)."""
    n = a.shape[0]
    if b_map:   # x = x_hi * 8 + h * 4 + j
        a = a.reshape(n, 4, 4, 4, 4, 2, 2, 4)  # z_hi z_lo y_hi y_lo x_hi h j
        a = a.transpose(0, 1, 3, 5, 6, 2, 4, 7)
    else:       # x = x_hi * 8 + j * 2 + h
        a = a.reshape(n, 4, 4, 4, 4, 2, 4, 2)  # z_hi z_lo y_hi y_lo x_hi j h
        a = a.transpose(0, 1, 3, 5, 7, 2, 4, 6)
    return a.reshape(n * 32, 2, 64)


def distinct(a):
    """distinct values along the last axis"""
    s = np.sort(a, axis=-1)
    return 1 + (s[..., 1:] != s[..., :-1]).sum(axis=-1)


per_instr = {False: [], True: []}
per_frame = {False: [], True: []}
live_all = []
n_blocks = 0
for k in range(0, 1000, 10):
    d, c, _, T = syn.render_frames(k, 1, W, H, device="cpu")
    d = d[0].numpy()
    keys = np.asarray(orc.depth_touch(d, K, np.asarray(T[0], np.float64), RES,
                                      VOX, TRUNC, DS, DMAX, 4), np.int64)
    n_blocks += len(keys)
    line, inb, zc, ui, vi = project(keys, T[0])
    df = d.astype(f32) / f32(DS)
    dd = np.where(inb, df[vi, ui], f32(0))
    ok = inb & (zc > 0) & (dd > 0) & (dd <= f32(DMAX)) & (dd - zc >= -f32(TRUNC))
    live_all.append(waves(ok, False).any(axis=(1, 2)))
    for b_map in (False, True):
        wl = waves(line, b_map)
        per_instr[b_map].append(distinct(wl))
        per_frame[b_map].append(distinct(wl.reshape(-1, 128)))

live = np.concatenate(live_all)
print("record-gather cache lines, bench stream, every 10th frame, %d x %d, "
      "res %d, %d-byte records, %d-byte lines" % (W, H, RES, REC, LINE))
print("block-frames %d (%.0f per frame), wave-frames issued %d, live (a voxel "
      "updates) %d = %.3f"
      % (n_blocks, n_blocks / 100, live.size, int(live.sum()), live.mean()))
res = {}
for b_map, name in ((False, "(A) x = 2j + h, today"),
                    (True, "(B) x = j + 4h")):
    pi = np.concatenate(per_instr[b_map])   # (wave-frames, 2)
    pf = np.concatenate(per_frame[b_map])   # (wave-frames,)
    for sel, what in ((slice(None), "issued"), (live, "live  ")):
        a, f = pi[sel], pf[sel]
        s = a.sum(axis=1)
        res[(b_map, what)] = s.mean()
        print("%-22s %s  lines per instruction: mean %.2f p90 %.0f (slot 0 "
              "%.2f, slot 1 %.2f);  per wave-frame: sum of the two %.2f (p90 "
              "%.0f), distinct of the two together %.2f (p90 %.0f)"
              % (name, what, a.mean(), np.percentile(a, 90), a[:, 0].mean(),
                 a[:, 1].mean(), s.mean(), np.percentile(s, 90), f.mean(),
                 np.percentile(f, 90)))
for what in ("issued", "live  "):
    print("line look-ups per wave-frame, (B) / (A), %s: %.3f"
          % (what, res[(True, what)] / res[(False, what)]))
