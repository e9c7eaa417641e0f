"""The collector's window rule and the oracle-side facts the GPU edge tests rest on (CPU).

tests/golden/collector_edges.npz holds the REFERENCE's _extract_patches and _check_boundaries at the corners and edge lines
of a 67x130 frame whose leaf reaches all of them (tests/golden/make_golden_collector.py edges).  The slices accept the
inclusive far edge x = W-16 / y = H-16; _check_boundaries refuses it, and the reference applies it to the positive point
only.  The oracle keeps the two rules apart (collector_extract_patches / collector_check_boundaries)."""
import os

import numpy as np
import pytest

from oracle import lg_oracle as O
from tests import collector_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
REGION_SHAPES = [(5, 7), (33, 47), (63, 65), (67, 130), (160, 224)]


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(HERE, "golden", "collector_edges.npz"))


def test_edges_fixture_holds_the_difference_between_the_two_rules(edges):
    H, W = int(edges["H"]), int(edges["W"])
    pts = [tuple(p) for p in edges["pts"].tolist()]
    assert (H, W) == (67, 130) and pts == CC.edges_points(H, W)
    assert pts[:4] == [(16, 16), (W - 16, 16), (16, H - 16), (W - 16, H - 16)]
    assert edges["ok"][:4].all()                                     # the slices are full at the inclusive far edge
    assert edges["bounds_ok"][:4].tolist() == [True, False, False, False]
    assert not edges["ok"][4:10].any() and not edges["bounds_ok"][4:10].any()
    np.testing.assert_array_equal(edges["mask"], CC.edges_mask())
    # accepted windows touch all four frame edges
    acc = [p for p, ok in zip(pts, edges["ok"]) if ok]
    assert any(x == 16 for x, _ in acc) and any(x == W - 16 for x, _ in acc)
    assert any(y == 16 for _, y in acc) and any(y == H - 16 for _, y in acc)


def test_oracle_window_rule_matches_reference_at_frame_edges(edges):
    mask, depth, scores = CC.edges_scene()
    np.testing.assert_array_equal(mask, edges["mask"])
    got = [O.collector_extract_patches(int(x), int(y), mask, depth, scores) for x, y in edges["pts"]]
    np.testing.assert_array_equal(np.array([g is not None for g in got]), edges["ok"])
    kept = [g for g in got if g is not None]
    np.testing.assert_array_equal(np.stack([g[0] for g in kept]), edges["depth"])
    np.testing.assert_array_equal(np.stack([g[1] for g in kept]), edges["mask_patches"])
    np.testing.assert_array_equal(np.stack([g[2] for g in kept]), edges["scores"])
    np.testing.assert_array_equal([O.collector_check_boundaries(int(x), int(y), mask.shape, 16) for x, y in edges["pts"]],
                                  edges["bounds_ok"])


def test_oracle_window_rule_exhaustive_on_a_small_frame():
    """Every centre of a 33x47 frame and a ring around it: accepted iff the NumPy slices are 32x32 and the coordinates
    are not negative; _check_boundaries is the same set without the far lines."""
    H, W = 33, 47
    rng = np.random.default_rng(0)
    mask = np.ones((H, W), np.uint8)
    depth = rng.random((H, W), dtype=np.float32)
    scores = {k: rng.random((H, W), dtype=np.float32) for k in O.SCORE_KEYS}
    for y in range(-20, H + 20):
        for x in range(-20, W + 20):
            full = x >= 16 and y >= 16 and depth[y - 16:y + 16, x - 16:x + 16].shape == (32, 32)
            assert (O.collector_extract_patches(x, y, mask, depth, scores) is not None) == full, (x, y)
            assert O.collector_check_boundaries(x, y, (H, W), 16) == (full and x != W - 16 and y != H - 16), (x, y)


@pytest.mark.parametrize("shape", REGION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_region_restatements_and_preconditions(shape):
    """The full-plane NumPy restatements the GPU test compares against agree with the oracle's point lists, and the
    masks do what their names say: two erosions leave nothing of the 5-px bar and a 1-px line of the 9-px bar, the
    straddling bar survives only below row int(0.75 H), the ridge's top-quarter cut falls inside a run of equal
    distances."""
    H, W = shape
    masks = CC.region_masks(H, W)
    q = int(0.75 * H)
    for name, m in masks.items():
        dist = O.distance_transform(m, 5)
        ys, xs = np.nonzero(CC.stem_plane(m))
        assert O.collector_stem_points(m) == list(zip(xs.tolist(), ys.tolist())), name
        ys, xs = np.nonzero(CC.tip_plane(m, dist))
        allp = list(zip(xs.tolist(), ys.tolist()))
        allp.sort(key=lambda p: dist[p[1], p[0]], reverse=True)
        assert O.collector_tip_points(m) == (allp[:max(1, len(allp) // 4)] if m.any() else []), name
        if name == "ridge" and min(H, W) >= 32:
            cut = max(1, len(allp) // 4)
            assert len(allp) > cut and dist[allp[cut - 1][1], allp[cut - 1][0]] == dist[allp[cut][1], allp[cut][0]]
    if W >= 11 and H - q >= 5:
        assert masks["bar5"][q:].sum(axis=1).tolist() == [5] * (H - q) and masks["bar9"][q:].sum(axis=1).tolist() == [9] * (H - q)
        assert O.collector_stem_points(masks["bar5"]) == []
        s9 = O.collector_stem_points(masks["bar9"])
        assert s9 and len({x for x, _ in s9}) == 1
        st = O.collector_stem_points(masks["straddle"])
        assert st and min(y for _, y in st) >= q + 4 and masks["straddle"][:q].any()
    assert O.collector_stem_points(masks["full"]) == [(x, y) for y in range(q + 4, H) for x in range(W)]
    if "cross64" in masks:
        xs = {x for x, _ in O.collector_stem_points(masks["cross64"])}
        assert min(xs) < 63 < 64 <= max(xs) or (W == 65 and 64 in xs)


def test_contour_preconditions():
    """The hand-made contour masks do what the GPU test needs: the 64x96 comb's contour does not fit the first buffer
    of _get_edge_points, of two equal components the first in raster order wins, area-0 components yield the first."""
    H, W = 64, 96
    ms = CC.contour_masks(H, W)
    assert len(O.leaf_contour_points(ms["comb"])) > 4 * (H + W) + 16
    for H, W in ((33, 47), (64, 96), (67, 130)):
        ms = CC.contour_masks(H, W)
        c = O.leaf_contour_points(ms["equal_pair"])
        assert c[0].tolist() == [3, 2] and c[:, 1].max() <= 5 and len(c) == 14
        assert O.leaf_contour_points(ms["area0"]).tolist() == [[1, 1]]
        assert O.leaf_contour_points(ms["pixel"]).tolist() == [[W // 3, H // 2]]
        line = O.leaf_contour_points(ms["line"])
        assert len(line) == 2 * (W - 4) - 2 and len(O.collector_edge_points(ms["line"])) == 2   # out and back
        assert len(O.leaf_contour_points(ms["full"])) == 2 * (H + W) - 4
        assert len(O.leaf_contour_points(ms["empty"])) == 0
