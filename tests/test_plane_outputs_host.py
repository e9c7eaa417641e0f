"""The premises of tests/test_gpu_plane_outputs.py, from the oracle and host arithmetic alone (no device): every case of
tests/plane_outputs.py has valid pixels and exactly top_k candidates; the `interior` cases, whose whole selection is held to
the oracle's, have no near-tie (the rule, the helpers and the bound of tests/test_oracle_params.py) at the seed the table
names, and every earlier seed misses the bound; the two frames hold every class of tile the plane kernel tells apart; and the
subsets are the ones the issue names, each mapped to the store form it reaches."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import near_tiles_ref as NT  # noqa: E402
from tests import param_oracle as PO  # noqa: E402
from tests import param_sets as PS  # noqa: E402
from tests import plane_outputs as PL  # noqa: E402

CASES = [(W, s, g) for W in PL.WIDTHS for s in PL.SCENES for g in PL.SIZES]


def _id(c):
    return f"{c[0]}-{c[1]}-g{c[2]}"


# ----------------------------------------------------------------------------- valid pixels, candidates
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_case_has_valid_pixels_and_top_k_candidates(case):
    W, name, g = case
    r = PL.run(W, name, g)
    n_valid = int(r["valid"].sum())
    print(f"{_id(case)}: {n_valid} valid, candidates {r['candidates']}, theta {r['theta']}")
    assert n_valid >= 8 and len(r["candidates"]) == PL.TOP_K
    assert r["theta"] is not None
    # no plane is all zero or constant on the leaf: nothing on the GPU compares zeros with zeros
    leaf = PL.mask_of(W, name) > 0
    for k in PL.PLANES:
        assert np.ptp(np.asarray(r["scores"][k], np.float64)[leaf]) > 0, k


def test_the_case_under_lg_default_params_has_valid_pixels():
    """p = NULL: the reference's constants, the camera at 707 / 494, f = 0 (unset) -- the approach plane is zero, the others are not"""
    for W in PL.WIDTHS:
        r = PL.run(W, "interior", 5, None, False, True)
        assert int(r["valid"].sum()) >= 8 and r["theta"] is not None
        assert not r["scores"]["approach_score"].any()
        leaf = PL.mask_of(W, "interior") > 0
        for k in PL.PLANES:
            if k != "approach_score":
                assert np.ptp(np.asarray(r["scores"][k], np.float64)[leaf]) > 0, k


def test_the_frames_and_the_constants_are_the_stated_ones():
    assert PL.H == 104 and PL.WIDTHS == (264, 263) and PL.SIZES == (1, 3, 5, 7)
    assert [W % 4 == 0 for W in PL.WIDTHS] == [True, False]
    for W in PL.WIDTHS:
        assert PL.tile_grid(W) == (5, 7) and W - 4 * PL.TW in (8, 7) and PL.H - 6 * PL.TH == 8
        m = PL.mask_of(W, "interior")
        assert NT.bbox(m) == (72, 207, 25, 79)
        c = PL.mask_of(W, "corner")
        assert c[0, 0] and c[:, W - 1].any() and not c[PL.H - 1].any()
        p = PL.params_of(W, 5)
        assert (p["top_k"], p["min_edge_distance"], p["nms_min_distance"], p["stem_se"], p["optimal_distance"],
                p["pregrasp_clearance"], p["w_flat"], p["flat_scale"]) == (4, 6, 6, 9, 10, 5, 1.0, 50)
        assert PS._STEEP == {"w_flat": 1.0, "flat_scale": 50}


# ----------------------------------------------------------------------------- no near-tie
def _gaps(W, g, seed, with_cnn):
    """(smallest relative gap of the walk, of the pick scores, the run)"""
    r = PL.run(W, "interior", g, seed, with_cnn)
    p = PL.params_of(W, g)
    if r["triple"][0] is None or len(r["candidates"]) != p["top_k"]:
        return 0.0, 0.0, r
    walk = PO.walk_gaps(r, p["top_k"], p["nms_min_distance"])
    assert len(walk) == len(r["candidates"])
    picks = np.unique(np.asarray(PO.pick_scores(r), np.float64))
    pick_gap = PO.smallest_relative_gap(picks) if picks.size > 1 else np.inf
    walk_gap = min((x for x, exact in walk if not exact), default=np.inf)
    return walk_gap, pick_gap, r


def _passes(W, g, seed):
    a, b = _gaps(W, g, seed, True), _gaps(W, g, seed, False)
    return min(a[0], a[1], b[0], b[1]) >= 1e-3 and a[2]["candidates"] == b[2]["candidates"], a, b


@pytest.mark.parametrize("g", PL.SIZES)
@pytest.mark.parametrize("W", PL.WIDTHS)
def test_interior_cases_have_no_near_tie(W, g):
    """tests/test_oracle_params.py::test_end_to_end_scenes_have_no_near_tie on these cases: at every pick of the walk the
    picked pixel and the best other pixel it could have taken, and any two deciding pick scores, lie 1e-3 relative apart or are
    the same float -- with the closed-form CNN and without it.  (One mask dtype: the GPU tests pass mask_is_bool = 1 only, and
    every candidate lies more than 16 px from the frame, so all are scored.)  The seed is the first of 0 .. 39 that passes."""
    seed = PL.SEEDS[(W, g)]
    ok, a, b = _passes(W, g, seed)
    print(f"{W} g={g} seed {seed}: walk {a[0]:.3g} / {b[0]:.3g}, pick scores {a[1]:.3g} / {b[1]:.3g} (with / without the CNN)")
    assert ok, (W, g, seed, a[:2], b[:2])
    assert all(m is not None for m in a[2]["ml_scores"])
    for x, y in a[2]["candidates"]:
        assert 16 <= x <= W - 16 and 16 <= y <= PL.H - 16
    for earlier in range(seed):
        assert not _passes(W, g, earlier)[0], (W, g, earlier)


def test_no_seed_serves_every_radius_at_264_and_none_does_without_the_steep_term():
    """why the table has one seed per (width, gaussian_size), and why the constants carry _STEEP"""
    assert not any(all(_passes(264, g, s)[0] for g in PL.SIZES) for s in range(max(PL.SEEDS.values()) + 1))
    assert len({PL.SEEDS[(264, g)] for g in PL.SIZES}) > 1
    from tests import frame_shapes as FS

    for W in PL.WIDTHS:     # the smooth terms alone leave less than 1e-3 between a pick and its runner-up
        mask, depth, P = PL.scene(W, "interior", PL.SEEDS[(W, 5)])
        p = dict(PL.params_of(W, 5), w_flat=FS.params_of(PL.H, W)["w_flat"], flat_scale=FS.params_of(PL.H, W)["flat_scale"])
        ref = PO.oracle(P, p)
        with np.errstate(all="ignore"):
            _, dbg = ref.select_grasp_point(mask, depth, return_debug=True)
        walk = PO.walk_gaps(dict(scores=dbg["scores"], valid=dbg["valid"], candidates=dbg["candidates"]), 4, 6)
        assert min(x for x, exact in walk if not exact) < 1e-3


# ----------------------------------------------------------------------------- tile classes
def _window(W, name):
    from tests.test_window_box_host import encode, lib_window

    return lib_window(encode(PL.mask_of(W, name)), PL.H, W, 2)[:4]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tile_classes(case):
    """Per case: far, near, stencil, constant tiles, tiles outside the sweep window, stencil tiles on the 16-byte staging path.
    `interior` has every class; `corner` has stencil tiles in tile row 0, tile column 0 and the last tile column."""
    W, name, g = case
    c = PL.tile_classes(W, name, g, _window(W, name))
    print(f"TILE-CLASSES {_id(case)}: " + " ".join(f"{k}={c[k]}" for k in ("far", "near", "stencil", "constant", "outside", "staged16")))
    assert c["far"] + c["near"] == 35 and c["stencil"] + c["constant"] == 35
    near, stencil, outside = c["near_map"], c["stencil_map"], c["outside_map"]
    if name == "interior":
        assert c["far"] > 0 and c["near"] > 0 and c["stencil"] > 0 and c["outside"] > 0 and c["staged16"] > 0
        # tile columns 0 and 4 and tile rows 0 and 6 stay off the stencil path at every radius
        assert not stencil[:, 0].any() and not stencil[:, 4].any() and not stencil[0].any() and not stencil[6].any()
        assert stencil[1:6, 1:4].any(axis=0).all()
        assert (outside & ~stencil).any()                      # distance = 0 written by the constant path
        assert (near & ~stencil).any()                         # a near tile whose bit-row test finds nothing (tile row 6)
    else:
        assert stencil[0].any() and stencil[:, 0].any() and stencil[:, 4].any()
        assert c["constant"] > 0
    # the partial last row and column exist and are written by some path in both scenes
    assert near.shape == (7, 5)


def test_the_window_leaves_tiles_outside_on_interior_only_where_stated():
    for W in PL.WIDTHS:
        wx0, wx1, wy0, wy1 = _window(W, "interior")
        assert (wx0, wy0, wy1) == (64, 16, 80) and wx1 == W    # columns from tile column 1 on, tile rows 1 to 4
        assert _window(W, "corner")[:1] == [0]


# ----------------------------------------------------------------------------- subsets and the forms they reach
def test_subsets():
    assert len(PL.EXHAUSTIVE) == 512 == len(set(PL.EXHAUSTIVE))
    assert len(PL.NAMED) == 2 + 8 + 8 + 2 and len({(p, v) for _, p, v in PL.NAMED}) == len(PL.NAMED)
    assert PL.FULL in PL.EXHAUSTIVE and PL.NOTHING in PL.EXHAUSTIVE
    forms = [PL.store_form(p, v) for p, v in PL.EXHAUSTIVE]
    # lg_score_maps: distance and traditional never decide the form (workspace planes stand in), validity never does
    assert forms.count("all") == 8 and forms.count("partial") == 504 and "score" not in forms
    named = {n: PL.store_form(p, v) for n, p, v in PL.NAMED}
    assert named["all planes, no validity"] == "all" and named["all but distance_map"] == "all"
    assert named["all but traditional_score"] == "all" and named["all but distance and traditional"] == "all"
    assert sum(f == "partial" for f in named.values()) == len(named) - 4
    # lg_select_grasp: nothing at all is the sparse, score-only form; a loaded model takes every workspace plane
    assert PL.store_form(*PL.NOTHING, entry="select") == "score"
    assert PL.store_form(frozenset([PL.SDF]), False, entry="select", model=True) == "all"
    assert PL.store_form(frozenset([PL.SDF]), False, entry="select") == "partial"
    assert PL.store_form(frozenset(), True, entry="select") == "partial"
    for W in PL.WIDTHS:
        for g in PL.SIZES:
            assert PL.instantiation(W, g, frozenset(), True) in PL.PARTIAL_FORMS
    assert len(PL.PARTIAL_FORMS) == 8
