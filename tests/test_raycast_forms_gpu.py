"""RayCastKernel in every form the host code launches it in, beyond the reach
of its LDS block table, and at poses that were never integrated -- pixels
against the oracle, or bit for bit against the form the rest of the suite
checks.

A workgroup tile is 32 x 8 pixels; o3dmi_internal_raycast_rows chooses from
the tile count (256 CUs, pinned by test_extension_loaded_and_device):
bands up to 1280 tiles, rounds (one workgroup per tile, the grid rounded up
to a multiple of 8) up to 4096, strided (4096 workgroups loop over the tiles
and clear their LDS block table in between) beyond; a grid-owned range map
adds the longest-first tile order to the rounds form and the range cells'
write-back to all of them; a row band shifts the tile rows. The recipes are
in _raycast_cases.py (test_raycast_cases_cpu.py checks that they are what
they claim), every cast goes through _raycast_poison.py: outputs filled with
NaN / 0x77 before the call, and no poison may be left after it."""
import functools

import numpy as np
import pytest
import torch

import _raycast_cases as rc
import _raycast_poison as poison
import _scene as sc

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open3d_amd import _lib, geometry
    return _lib, geometry


@functools.lru_cache(maxsize=None)
def _device_grid(res, grid_f32):
    """The device twin of rc.grid(res, grid_f32): same frames, same keys.
    Shared between the tests (ray casts do not write to a grid)."""
    from test_vbg_gpu import _mk_grid
    _, geometry = _gpu()
    _, _, per_frame, _ = rc.grid(res, grid_f32)
    g = _mk_grid(geometry, grid_f32, block_count=rc.GRID_CAPACITY[res],
                 res=res)
    for k, keys in zip(rc.FRAMES, per_frame):
        d, c, K, Ts = sc.frames(k, 1, rc.FRAME_W, rc.FRAME_H)
        g.integrate(torch.from_numpy(keys).cuda(),
                    torch.from_numpy(d[0]).cuda(),
                    torch.from_numpy(c[0]).cuda(), K, K, Ts[0],
                    sc.DEPTH_SCALE, sc.DEPTH_MAX, sc.TRUNC_MULT)
    return g


def _cast(cs, g, attrs):
    """The case's poisoned cast: explicit keys, caller's range map."""
    got = poison.ray_cast(g, torch.from_numpy(cs.keys).cuda(), cs.K, cs.T,
                          cs.w, cs.h, attrs, sc.DEPTH_SCALE, cs.depth_min,
                          cs.depth_max, rc.WEIGHT_THRESHOLD, sc.TRUNC_MULT,
                          rc.DOWN)
    return {a: t.cpu().numpy() for a, t in got.items()}


def _assert_parity(cs, g, want_range, want, got, depth_tol=1e-3,
                   vertex_tol=1e-5, report=None):
    """test_raycast_parity's assertions for whichever maps `want` holds."""
    worst = {}
    if "range" in got:
        assert np.array_equal(got["range"], want_range)
    for a in want:
        if a == "mask":
            assert np.array_equal(got[a].astype(bool), want[a])
        elif a != "index":
            if a == "depth":
                assert np.array_equal(got[a] > 0, want[a] > 0)
            worst[a] = float(np.abs(got[a] - want[a]).max())
    if report:
        print("%s: worst error %s" % (report, ", ".join(
            "%s %.3g" % kv for kv in sorted(worst.items()))))
    for a, err in worst.items():
        tol = depth_tol if a == "depth" else (  # depth units (mm)
            vertex_tol if a == "vertex" else 1e-5)
        assert err <= tol, (a, err)
    if "index" in want:
        # voxel indices are buffer-index based: compare through the key of
        # the block they point into (under the oracle's mask, which an
        # `index`-only cast has no other way to be checked against)
        res3 = cs.res ** 3
        _, full = rc.oracle_maps(cs.name, cs.og.weight.dtype == np.float32,
                                 rc.ALL_ATTRS)
        m = full["mask"]
        gi, wi = got["index"], want["index"]
        gk = g.hashmap().key_tensor().cpu().numpy()[(gi // res3)[m]]
        wk = cs.og.h.key_buffer()[(wi // res3)[m]]
        assert np.array_equal(gk, wk)
        assert np.array_equal((gi % res3)[m], (wi % res3)[m])
        assert not gi[~m].any()


# ---- (a) the forms against the oracle

@pytest.mark.parametrize("grid_f32", [False, True])
@pytest.mark.parametrize("name", ["rounds", "strided"])
def test_rounds_and_strided_forms_equal_the_oracle(name, grid_f32):
    """1353 tiles: a grid of 1360 workgroups, 7 of which have no tile. 4141
    tiles: 4096 workgroups, 45 of which render a second tile. The last tile
    column is 24 pixels wide, so wave 3 of its workgroups has no ray."""
    _gpu()
    cs = rc.case(name, grid_f32)
    g = _device_grid(cs.res, grid_f32)
    want_range, want = rc.oracle_maps(name, grid_f32)
    got = _cast(cs, g, rc.MAPS)
    _assert_parity(cs, g, want_range, want, got)


def test_strided_form_full_kernel_equals_the_oracle():
    """The FULL instantiation (index / mask / interp_ratio*) in the strided
    loop: all ten attributes."""
    _gpu()
    cs = rc.strided()
    g = _device_grid(cs.res, False)
    want_range, want = rc.oracle_maps("strided", False, rc.ALL_ATTRS)
    got = _cast(cs, g, rc.ALL_ATTRS)
    _assert_parity(cs, g, want_range, want, got)


# ---- (b) ordered rounds and the self-cleaning range map

_LIMITS = {"rounds": ((0.1, 3.0), (0.1, 3.0), (0.3, 2.0), (0.1, 3.0),
                      (0.1, 3.0)),
           "strided": ((0.1, 3.0), (0.1, 3.0), (0.3, 2.0))}


@pytest.mark.parametrize("name", ["rounds", "strided"])
def test_grid_owned_casts_equal_the_callers_map_casts_bit_for_bit(name):
    """o3dmi_vbg_ray_cast_dev without keys and without a range map, at sizes
    beyond the bands form. At the `rounds` size workgroup k renders
    tile_order[k], sorted (by one extra workgroup of the range-estimate
    launch) from the tile costs the PREVIOUS cast left -- which was at another
    pose, so the order is far from the identity and far from this view's
    costs; "which tile a workgroup renders changes no pixel". At the
    `strided` size no order is used, but the map still resets itself, tile
    after tile. Before each cast one more frame is integrated; the pose
    alternates between that frame's and its novel_c variant, so successive
    range maps differ widely; the depth limits change and change back (the
    map must be refilled); every grid-owned cast is followed by a cast with
    a caller's map, which must not disturb the next one. Each result is bit
    for bit the caller's-map cast of the same keys, pose and limits.

    Limit of this check: a range cell left dirty only WIDENS a ray's
    interval. That changes pixels through the phase of the march's samples
    alone -- which bit-equality catches for most rays, not provably for all
    of them."""
    _, geometry = _gpu()
    from test_vbg_gpu import _mk_grid
    cs = rc.case(name)
    _, _, _, yaw, shift, back, _, _ = rc.RECIPES["novel_c"]
    g = _mk_grid(geometry, False, block_count=16384)
    cap = (rc.FRAME_H // 4) * (rc.FRAME_W // 4) * 4
    for i, lim in enumerate(_LIMITS[name]):
        d, c, K, Ts = sc.frames(300 + 2 * i, 1, rc.FRAME_W, rc.FRAME_H)
        g.integrate_frame(torch.from_numpy(d[0]).cuda(),
                          torch.from_numpy(c[0]).cuda(), K, K, Ts[0],
                          sc.DEPTH_SCALE, sc.DEPTH_MAX, sc.TRUNC_MULT)
        T = Ts[0] if i % 2 == 0 else rc.novel_pose(Ts[0], yaw, shift, back)
        own = poison.ray_cast_last_frame(
            g, cs.K, T, cs.w, cs.h, rc.MAPS, sc.DEPTH_SCALE, lim[0], lim[1],
            rc.WEIGHT_THRESHOLD, sc.TRUNC_MULT, rc.DOWN)
        coords, cnt = g.last_frame_block_coordinates(cap)
        keys = coords[:int(cnt.item())].contiguous()
        ref = poison.ray_cast(
            g, keys, cs.K, T, cs.w, cs.h, rc.MAPS, sc.DEPTH_SCALE, lim[0],
            lim[1], rc.WEIGHT_THRESHOLD, sc.TRUNC_MULT, rc.DOWN)
        hit = float((ref["depth"] > 0).float().mean())
        print("%s cast %d, limits %s: hit share %.3f" % (name, i, lim, hit))
        # (a guard against an empty image, not a measurement: the oracle
        # gives 0.44 for novel_c over the union of four frames' blocks)
        assert hit > 0.2, (i, hit)
        for a in rc.MAPS:
            assert torch.equal(own[a].view(torch.int32),
                               ref[a].view(torch.int32)), (a, i, lim)


# ---- (c) row bands outside the bands form

def _assert_band(whole, band, r0, r1):
    for a, t in band.items():
        assert torch.equal(t[r0:r1].view(torch.int32),
                           whole[a][r0:r1].view(torch.int32)), (a, r0, r1)
        assert bool(poison.poisoned(a, t[:r0]).all()), (a, r0, r1)
        assert bool(poison.poisoned(a, t[r1:]).all()), (a, r0, r1)


@pytest.mark.parametrize("name,bands", [
    ("strided", ((0, 264), (264, 536), (536, 808))),  # 41 * 33 / 34 tiles
    ("rounds", ((8, 16),)),                           # one tile row: bands
])
def test_row_bands_equal_the_rows_of_the_whole_image(name, bands):
    """o3dmi_vbg_raycast_rows with a non-zero first tile row, in the rounds
    form (thirds of the strided image) and for one tile row: inside the band
    the maps are the whole-image cast's bit for bit, outside it the poison
    is untouched."""
    _gpu()
    cs = rc.case(name)
    g = _device_grid(cs.res, False)
    whole = poison.ray_cast(g, torch.from_numpy(cs.keys).cuda(), cs.K, cs.T,
                            cs.w, cs.h, rc.MAPS, sc.DEPTH_SCALE, cs.depth_min,
                            cs.depth_max, rc.WEIGHT_THRESHOLD, sc.TRUNC_MULT,
                            rc.DOWN)
    for r0, r1 in bands:
        band = poison.ray_cast_rows(
            g, whole["range"], cs.K, cs.T, cs.w, cs.h, r0, r1, rc.MAPS,
            sc.DEPTH_SCALE, cs.depth_min, cs.depth_max, rc.WEIGHT_THRESHOLD,
            sc.TRUNC_MULT, rc.DOWN)
        _assert_band(whole, band, r0, r1)


# ---- (d) blocks the LDS table refuses

@pytest.mark.parametrize("grid_f32", [False, True])
@pytest.mark.parametrize("name", ["far", "far_neg"])
def test_far_blocks_bypass_the_lds_table(name, grid_f32):
    """8^3 blocks of 8 mm voxels seen through a telephoto lens from 6.5 m
    further back: the hit blocks are 118 to 129 blocks from the camera's own
    on +x, on both sides of the 128 LdsBlockTable::Encode accepts, so the
    table and its bypass serve one image. `far_neg` has them 98 to 138 blocks
    away on -z: Encode's offsets are unsigned, and it is a NEGATIVE y or z
    offset that, let into the table, would alias other blocks' entries.
    Depth and vertex errors grow with the range: the 1e-3 depth units at 3 m
    are 3.3e-7 of the range, which is 4e-3 depth units and 4e-5 m at 12 m.

    Measured on an MI355X, both cases and both grid dtypes: every map equals
    the oracle's bit for bit (worst errors 0; the figures are printed)."""
    _gpu()
    cs = rc.case(name, grid_f32)
    g = _device_grid(cs.res, grid_f32)
    want_range, want = rc.oracle_maps(name, grid_f32)
    got = _cast(cs, g, rc.MAPS)
    _assert_parity(cs, g, want_range, want, got, depth_tol=4e-3,
                   vertex_tol=4e-5,
                   report="%s, %s grid" % (name, "f32" if grid_f32 else "u16"))


# ---- (e) novel views

@pytest.mark.parametrize("grid_f32", [False, True])
@pytest.mark.parametrize("name", ["novel_a", "novel_b", "novel_c"])
def test_novel_views_equal_the_oracle(name, grid_f32):
    """Poses that were never integrated: oblique views, rays that leave the
    allocated blocks sideways, image parts without any block. All ten
    attributes, test_raycast_parity's assertions."""
    _gpu()
    cs = rc.case(name, grid_f32)
    g = _device_grid(cs.res, grid_f32)
    want_range, want = rc.oracle_maps(name, grid_f32, rc.ALL_ATTRS)
    got = _cast(cs, g, rc.ALL_ATTRS)
    _assert_parity(cs, g, want_range, want, got)


# ---- (f) attribute subsets

@pytest.mark.parametrize("attrs", [
    ("depth",), ("vertex",), ("normal",), ("color",), ("mask",), ("index",),
    ("interp_ratio_dz",), ("depth", "mask")], ids="+".join)
def test_attribute_subsets_equal_the_oracle(attrs):
    """The slim kernel without visit_neighbors (depth or vertex alone), and
    the FULL kernel with a single output pointer set."""
    _gpu()
    cs = rc.novel_a()
    g = _device_grid(cs.res, False)
    want_range, full = rc.oracle_maps("novel_a", False, rc.ALL_ATTRS)
    got = _cast(cs, g, attrs)
    assert set(got) == set(attrs) | {"range"}
    _assert_parity(cs, g, want_range, {a: full[a] for a in attrs}, got)
