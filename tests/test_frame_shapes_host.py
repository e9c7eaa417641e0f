"""The premises of tests/test_gpu_frame_shapes.py, from the oracle and host arithmetic alone (no device): every case of
tests/frame_shapes.py has valid pixels and the stated number of candidates, so nothing on the GPU compares zeros with zeros;
the end-to-end cases have no near-tie (the rule and the helper of tests/test_oracle_params.py); and the table of shapes reaches
every path it is meant to reach -- the forms of the row search (lg_dt_form_host), the sweep geometries, the word and tile
counts at their limits, a CNN window larger than the frame."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import frame_shapes as FS  # noqa: E402
from tests import param_oracle as PO  # noqa: E402

SMALL_AND_WIDE = FS.SMALL + FS.WIDE_TALL


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


# ----------------------------------------------------------------------------- valid pixels, candidate counts
@pytest.mark.parametrize("shape", SMALL_AND_WIDE, ids=_id)
def test_every_case_has_valid_pixels_and_its_candidates(shape):
    """The two degenerate masks (a line one pixel wide, the empty mask) have no valid pixel by construction and are held to
    exactly that: their candidates are the fall-through picks."""
    kinds = set()
    for case in FS.plane_cases(shape):
        r = FS.run(case)
        n_valid = int(r["valid"].sum())
        print(f"{case.name}: {n_valid} valid, {len(r['candidates'])} candidates")
        if case.kind in FS.DEGENERATE:
            assert n_valid == 0, case.name
        else:
            assert n_valid >= 8, (case.name, n_valid)
        assert len(r["candidates"]) == case.n_cand == case.top_k, case.name
        kinds.add(case.kind)
    long = {"ends", "corner"}
    assert kinds >= set(FS.MASKS) - long and ((kinds >= long) == FS.applicable(*shape, "ends"))


def test_frames_that_run_out_of_candidates():
    """top_k above what the frame can space: the walk stops early, with the count the table states (8-row frames)."""
    assert len(FS.RUN_OUT) >= 2
    for case in FS.RUN_OUT:
        r = FS.run(case)
        assert int(r["valid"].sum()) >= 16
        assert len(r["candidates"]) == case.n_cand < case.top_k, (case.name, len(r["candidates"]))
        assert min(case.shape) <= 9


# ----------------------------------------------------------------------------- no near-tie on the end-to-end cases
@pytest.mark.parametrize("case", FS.END_TO_END, ids=lambda c: c.name)
@pytest.mark.parametrize("mask_is_bool", [1, 0], ids=["bool", "uint8"])
def test_end_to_end_cases_have_no_near_tie(case, mask_is_bool):
    """tests/test_oracle_params.py::test_end_to_end_scenes_have_no_near_tie, on these frames: same helper, same bound."""
    params = case.params(mask_is_bool=mask_is_bool)
    r = FS.run(case, True, mask_is_bool)
    assert r["triple"][0] is not None and len(r["candidates"]) == params["top_k"]
    walk = PO.walk_gaps(r, params["top_k"], params["nms_min_distance"])
    assert len(walk) == len(r["candidates"])
    picks = np.unique(np.asarray(PO.pick_scores(r), np.float64))
    pick_gap = PO.smallest_relative_gap(picks) if picks.size > 1 else np.inf
    walk_gap = min((g for g, exact in walk if not exact), default=np.inf)
    print(f"{case.name}: smallest gap of the walk {walk_gap:.3g}, of the pick scores {pick_gap:.3g}")
    assert walk_gap >= 1e-3 and pick_gap >= 1e-3, (case.name, walk_gap, pick_gap)
    assert FS.run(case, False, mask_is_bool)["candidates"] == r["candidates"]
    scored = [m is not None for m in r["ml_scores"]]
    if mask_is_bool and not FS.window_fits(*case.shape):
        assert not any(scored)          # no 32 x 32 window fits: a bool mask scores nothing
    if not mask_is_bool:
        assert all(scored)              # a uint8 mask: every candidate, replicated over the border


def test_every_shape_has_one_end_to_end_case():
    assert sorted(FS.E2E_BY_SHAPE) == sorted(SMALL_AND_WIDE) and len(FS.END_TO_END) == len(SMALL_AND_WIDE)
    assert FS.LARGE not in FS.E2E_BY_SHAPE


# ----------------------------------------------------------------------------- the paths the table reaches
def _form(forced, H, W, n=1):
    from leafgrasp_amd import _lib

    return int(_lib.lib.lg_dt_form_host(forced, n, H, W))


def test_the_table_reaches_every_path_it_is_meant_to():
    tags = {}
    for H, W in FS.SHAPES:
        for t in FS.reach(H, W):
            tags.setdefault(t, []).append((H, W))
    for t in ("form1_forced", "sixteen", "W_2049_4096", "W_4097_8191", "W_8192", "H_16384", "tiles_8192", "one_tile",
              "one_word_tail", "window_over_all_borders", "hrun_pieces", "iso_sweep_32"):
        assert tags.get(t), t
    # forms 5 and 6 at exactly sixteen rows or columns, form 1 forced below (whatever LG_DT_SEARCH_ALGO asks for)
    for H, W in tags["form1_forced"]:
        assert _form(5, H, W) == 1 and _form(6, H, W) == 1 and _form(0, H, W, 1 << 20) == 1, (H, W)
    assert (16, 16) in tags["sixteen"] and (16, 64) in tags["sixteen"] and (16384, 16) in tags["sixteen"]
    for H, W in tags["sixteen"]:
        assert _form(5, H, W) == 5 and _form(6, H, W) == 6, (H, W)
    for H, W in FS.SHAPES:   # the register sweep ends at 2048 columns; one frame of any of these is a small batch
        if H >= 16 and W >= 16:
            assert _form(6, H, W) == (6 if W <= 2048 else 5) and _form(5, H, W) == 5, (H, W)
        assert _form(0, H, W) == 1 and _form(1, H, W) == 1
    # the sweep workgroup: 512 x 8 up to 4096 columns, 1024 x 8 above (lg_dt5_kernel<1024, 8, *, *>)
    assert FS.sweep_geometry(2112) == (512, 8) and FS.sweep_geometry(4160) == (1024, 8) and FS.sweep_geometry(8192) == (1024, 8)
    assert FS.sweep_geometry(8129) == (1024, 8)
    assert FS.words(4160) == 65 and FS.words(8192) == 128 and FS.words(8129) == 128 and FS.words(2112) == 33
    assert FS.tiles(*FS.LARGE) == 8192 and FS.LARGE[1] > 4096
    assert FS.tiles(16384, 8) == 1024 and FS.tiles(8, 8) == 1 and FS.tiles(17, 65) == 4
    assert {(8, 8), (8, 9), (9, 8), (8, 63), (15, 64), (16, 16)} <= set(tags["one_tile"]) | set(tags["one_word_tail"])
    assert (8, 8) in tags["window_over_all_borders"] and (16, 16) in tags["window_over_all_borders"]
    assert not FS.window_fits(31, 33) and not FS.window_fits(33, 31) and FS.window_fits(200, 12) is False


def test_what_make_plan_refuses_lies_just_outside_the_table():
    """the refusals of tests/test_gpu_frame_shapes.py, next to the admitted shapes they border on"""
    assert FS.tiles(16384, 520) == 9216 > 8192 >= FS.tiles(16384, 512)
    for H, W in FS.SHAPES:
        assert 8 <= H <= 16384 and 8 <= W <= 8192 and FS.tiles(H, W) <= 8192
    for H, W in FS.REFUSED_SHAPES:
        assert H < 8 or W < 8 or W > 8192 or H > 16384 or FS.tiles(H, W) > 8192


def test_frames_where_a_distance_reaches_init_dist0():
    """OpenCV's border cells hold chamfer_init_dist0 (INT_MAX >> 2 = 8192 px) and cap the transform there: only the frames of
    16384 rows or 8192 columns (and the large one) can tell, under INT_MAX none does -- and on the corner mask of 16384 x 8 the
    oracle's largest d_out is the capped 8196, not the 16376.6 px to the far corner."""
    from oracle import lg_oracle as O

    far = [s for s in FS.SHAPES if FS.far(*s)]
    assert sorted(far) == sorted([(24, 8192), (8, 8192), (16384, 8), (16384, 16), FS.LARGE])
    assert not any(FS.far(*s, FS.INT_MAX) for s in FS.SHAPES)
    assert FS.norm5(3, 4) == 143976 + 2 * 91750 and FS.norm5(10, 2) == 6 * 65536 + 2 * 143976
    m = FS.mask_of(16384, 8, "corner")
    d = O.distance_transform(1 - m, 5)
    assert d.max() == 8196.0
    assert abs(float(O.distance_transform(1 - m, 5, init_dist0=FS.INT_MAX).max()) - 16376.59) < 0.01
