"""The ray-cast cases of _raycast_cases.py test what they claim -- on the
oracle alone, no GPU. These conditions are not measurements: they keep a GPU
test from passing on an image with nothing in it, or on a `far` image whose
blocks all lie on one side of the LDS block table's 128-block reach."""
import numpy as np
import pytest

import _raycast_cases as rc


def _hit_share(name):
    _, want = rc.oracle_maps(name)
    return float((want["depth"][..., 0] > 0).mean())


# The thresholds between the forms are 5 and 16 tiles per CU with kCUs = 256
# (test_vbg_gpu.test_extension_loaded_and_device pins the 256).
@pytest.mark.parametrize("name,tiles,form", [("rounds", 1353, "rounds"),
                                             ("strided", 4141, "strided")])
def test_large_cases_cross_the_form_thresholds_and_hit(name, tiles, form):
    cs = rc.case(name)
    assert rc.tile_count(cs.w, cs.h) == tiles
    assert rc.launch_form(cs.w, cs.h) == form
    assert 5 * rc.CUS < 1353 <= 16 * rc.CUS < 4141
    # the last tile column is 24 pixels wide: wave 3 of its workgroups has
    # no ray; the range map's cells are whole
    assert cs.w % 32 == 24 and cs.w % 8 == 0 and cs.h % 8 == 0
    share = _hit_share(name)
    print("%s: hit share %.3f" % (name, share))
    assert share > 0.9, share


def test_row_bands_of_the_strided_image_are_rounds_launches():
    cs = rc.strided()
    for r0, r1 in ((0, 264), (264, 536), (536, 808)):
        assert r0 % 8 == 0 and r1 % 8 == 0
        assert rc.launch_form(cs.w, r1 - r0) == "rounds"


@pytest.mark.parametrize("name", ["novel_a", "novel_b", "novel_c"])
def test_novel_views_have_many_hits_and_many_misses(name):
    cs = rc.case(name)
    assert rc.launch_form(cs.w, cs.h) == "bands"
    share = _hit_share(name)
    print("%s: hit share %.3f" % (name, share))
    assert 0.3 <= share <= 0.9, share


def test_far_case_serves_the_block_table_and_its_bypass():
    cs = rc.far()
    assert rc.launch_form(cs.w, cs.h) == "bands"
    _, want = rc.oracle_maps("far")
    hit = want["depth"][..., 0] > 0
    assert hit.mean() > 0.9, hit.mean()
    dist = rc.block_distance(cs, want["vertex"], hit)
    beyond = float((dist >= 128).mean())
    print("far: hit share %.3f, %.1f %% of the hits at 128 blocks or more, "
          "distances %d .. %d blocks" % (hit.mean(), 100 * beyond, dist.min(),
                                         dist.max()))
    assert beyond >= 0.05, beyond
    assert 1 - beyond >= 0.05, beyond


def test_far_neg_case_leaves_the_table_on_a_negative_axis():
    """Many hits and many misses, as in the novel views; of the hit blocks
    at least 5 % below -128 on z and at least 5 % inside the table, and no
    axis past +127 (that is `far`)."""
    cs = rc.far_neg()
    assert rc.launch_form(cs.w, cs.h) == "bands"
    _, want = rc.oracle_maps("far_neg")
    hit = want["depth"][..., 0] > 0
    assert 0.3 <= hit.mean() <= 0.9, hit.mean()
    off = rc.block_offsets(cs, want["vertex"], hit)
    below = float((off[:, 2] < -128).mean())
    print("far_neg: hit share %.3f, %.1f %% of the hits below -128 on z, "
          "offsets x %d .. %d, y %d .. %d, z %d .. %d" % (
              hit.mean(), 100 * below, off[:, 0].min(), off[:, 0].max(),
              off[:, 1].min(), off[:, 1].max(), off[:, 2].min(),
              off[:, 2].max()))
    assert below >= 0.05 and 1 - below >= 0.05, below
    assert off.max() < 128 and off[:, :2].min() >= -128


def test_grids_fit_and_keys_are_the_union_of_the_frames():
    for res in (16, 8):
        og, keys, per_frame, _ = rc.grid(res, False)
        assert og.h.size() == keys.shape[0] <= rc.GRID_CAPACITY[res]
        assert len(per_frame) == 4
        assert keys.shape[0] > max(k.shape[0] for k in per_frame)
