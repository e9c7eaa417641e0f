"""collect_sample end to end where the suite could not see an error before (-m gpu).

  * The tip points follow the MASK.  The reference's _get_tip_points (data_collector.py:421-441) recomputes
    cv2.distanceTransform(mask); scores['distance_map'] only fills the score patches.  Handing in a plane that is not the
    transform of this mask -- (a) the true transform times 0.5, (b) the transform of another leaf -- must not move the
    tip points.  (a) keeps local maxima and their order, so it held before the collector derived the tips from the mask;
    (b) did not.
  * The two window rules.  (W-16, H-16) is refused as a positive (_check_boundaries :83-89, :203) and taken as a
    negative (:332 goes straight to _extract_patches, whose slices are full there).
Expected samples: tests/collector_cases.replay_collect_sample, a NumPy replay of :175-348 on the oracle's helpers with
the same `random` seed; patches are compared bit for bit."""
import random

import numpy as np
import pytest

from oracle import lg_oracle as O
from tests import collector_cases as CC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 7          # chosen on the CPU: the accepted negatives of case (b) are tip, stem, tip (see the assertion there)
CORNER_SEED = 3   # no influence on the points here (one tip point, no stem or edge points); fixed all the same


@pytest.fixture(scope="module")
def collector(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import leafgrasp_amd as L

    return L.EnhancedGraspDataCollector(patch_size=32, resume=False, data_dir=str(tmp_path_factory.mktemp("lg_collect")),
                                        device="cuda:0")


@pytest.fixture(scope="module")
def scene():
    leaf, other = CC.collect_scene_masks()
    depth, scores = CC.scene_scores(leaf, 12)
    np.testing.assert_array_equal(scores["distance_map"], O.distance_transform(leaf, 5))   # what a caller normally hands in
    return leaf, other, depth, scores


def _run(collector, mask, depth, scores, point, total, seed):
    collector.samples, collector.stats = [], {"positive_samples": 0, "negative_samples": 0, "augmented_samples": 0}
    dev = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in scores.items()}
    random.seed(seed)
    return collector.collect_sample(torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(depth).cuda(), None, dev,
                                    point, total)


def _same(samples, exp):
    assert [s["grasp_point"] for s in samples] == [tuple(e[1]) for e in exp]
    assert len(samples) == len(exp)
    for s, (p, pt, tot, lab, _) in zip(samples, exp):
        assert s["label"] == lab and abs(s["total_score"] - tot) < 1e-12
        np.testing.assert_array_equal(s["mask_patch"].numpy(), p[1])
        np.testing.assert_array_equal(s["score_patches"].numpy(), p[2])
        if not s["is_augmented"]:
            np.testing.assert_array_equal(s["depth_patch"].numpy(), p[0])


def _wrong_tips(mask, plane):
    """What a collector that took the handed plane for the transform of the mask would draw its tips from."""
    ys, xs = np.nonzero(CC.tip_plane(mask, plane))
    pts = list(zip(xs.tolist(), ys.tolist()))
    pts.sort(key=lambda p: plane[p[1], p[0]], reverse=True)
    return pts[:max(1, len(pts) // 4)]


@pytest.mark.parametrize("case", ["half", "other_leaf"])
def test_tip_points_follow_the_mask_not_the_handed_distance_plane(collector, scene, case):
    leaf, other, depth, scores = scene
    true = scores["distance_map"]
    handed = true * np.float32(0.5) if case == "half" else O.distance_transform(other, 5)
    assert not np.array_equal(handed, true)
    sc = dict(scores, distance_map=handed)
    exp = CC.replay_collect_sample(leaf, depth, sc, (110, 120), 0.75, SEED)
    assert exp is not None
    negs = [e for e in exp if e[3] == 0]
    tips = [e[1] for e in negs if e[4] == "tip"]
    assert len(negs) == 3 and tips and all(t in O.collector_tip_points(leaf) for t in tips)
    if case == "other_leaf":                               # the foreign plane would have led somewhere else entirely
        assert not set(_wrong_tips(leaf, handed)) & set(O.collector_tip_points(leaf))
    else:                                                  # exact scaling keeps every comparison: same tips either way
        assert _wrong_tips(leaf, handed) == O.collector_tip_points(leaf)
    ch = O.SCORE_KEYS.index("distance_map")
    np.testing.assert_array_equal(exp[0][0][2][ch], handed[120 - 16:120 + 16, 110 - 16:110 + 16])   # patches: the handed plane
    assert _run(collector, leaf, depth, sc, (110, 120), 0.75, SEED)
    _same(collector.samples, exp)


def test_far_corner_is_refused_as_a_positive_and_taken_as_a_negative(collector):
    mask, depth, scores = CC.corner_scene()
    H, W = mask.shape
    corner = (W - 16, H - 16)
    assert (H, W) == (67, 130) and O.collector_tip_points(mask) == [corner]
    assert not O.collector_stem_points(mask) and not O.collector_edge_points(mask)
    assert O.collector_extract_patches(*corner, mask, depth, scores) is not None
    assert not O.collector_check_boundaries(*corner, mask.shape, 16)
    # as a positive: refused, nothing collected
    assert CC.replay_collect_sample(mask, depth, scores, corner, 0.5, CORNER_SEED) is None
    assert _run(collector, mask, depth, scores, corner, 0.5, CORNER_SEED) is False
    assert collector.samples == [] and sum(collector.stats.values()) == 0
    # one pixel in: the positive is taken, and the corner comes back as every negative
    exp = CC.replay_collect_sample(mask, depth, scores, (W - 17, H - 17), 0.5, CORNER_SEED)
    assert [e[1] for e in exp if e[3] == 0] == [corner] * 3
    assert _run(collector, mask, depth, scores, (W - 17, H - 17), 0.5, CORNER_SEED)
    _same(collector.samples, exp)
    assert collector.stats == {"positive_samples": 1, "negative_samples": 3, "augmented_samples": 3}
