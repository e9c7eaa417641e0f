"""The grasp path with the CNN at the benchmark's own batch: 256 frames of 1080p, 5120 candidate patches through the CNN at
once, every frame against the single-frame call of its scene and four scenes against the float64 oracle.  And a batch whose
candidate patches exceed the CNN's slice of 8192 (lg_select_grasp cuts the haloed patches into slices)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests.test_gpu_grasp_candidates import _assert_rows_match_oracle, _by_index, _oracle_rows, _params, _valid_rows  # noqa: E402

EXACT = ("index", "x", "y", "traditional", "scored", "X", "Y", "Z", "has_pre", "pX", "pY", "pZ")
CLOSE = ("ml_score", "ml_confidence", "combined")


@pytest.fixture(scope="module")
def sel():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    s.set_cnn_state_dict(_params())
    yield s
    s.clear_cnn()


@functools.lru_cache(maxsize=None)
def _headline_frames():
    import bench

    return bench.make_frames(256, 1080, 1920, workers=1)


def _largest_leaf(labels):
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    return labels == ids[np.argmax(counts)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _order_differs_only_at_near_ties(rb, rs):
    """Rank order of a batch frame (rb) against its single call (rs): equal, or equal up to a pick whose deciding pick scores
    lie within 1e-5 relative.  Returns True when the orders differ."""
    ib, is_ = rb["index"].tolist(), rs["index"].tolist()
    if ib == is_:
        np.testing.assert_array_equal(rb["by_ml"], rs["by_ml"])
        np.testing.assert_allclose(rb["pick_score"], rs["pick_score"], rtol=1e-5, atol=1e-6, equal_nan=True)
        return False
    r = next(i for i, (a, b) in enumerate(zip(ib, is_)) if a != b)
    assert ib[:r] == is_[:r] and (rb["by_ml"][:r] == rs["by_ml"][:r]).all(), r
    np.testing.assert_allclose(rb["pick_score"][:r + 1], rs["pick_score"][:r + 1], rtol=1e-5, atol=1e-6, equal_nan=True)
    # the two picks at rank r: the batch's winner, as scored in the single call, came within 1e-5 of the single call's winner
    s_win = float(rs["pick_score"][r])
    alt = _by_index(rs)[ib[r]]
    own = max(float(alt["traditional"]), float(alt["combined"]) if alt["scored"] else -np.inf)
    assert abs(own - s_win) <= 1e-5 * max(abs(s_win), 1e-30), (r, ib[r], is_[r], own, s_win)
    return True


def _assert_frame_equals_single(rb, rs, what):
    assert len(rb) == len(rs), what
    xb, xs = _by_index(rb), _by_index(rs)
    for f in EXACT:
        np.testing.assert_array_equal(xb[f], xs[f], err_msg=f"{what} {f}")
    for f in CLOSE:
        np.testing.assert_allclose(xb[f], xs[f], rtol=1e-5, atol=1e-6, equal_nan=True, err_msg=f"{what} {f}")
    return _order_differs_only_at_near_ties(rb, rs)


def test_headline_batch_256_frames_1080p(sel):
    masks, depths, P, _ = _headline_frames()
    n_scenes = 32
    B = masks.shape[0]
    assert B == 256
    sel.set_camera_params(P)
    m, d = _dev(masks), _dev(depths)
    # (a) the candidates entry's results are lg_select_grasp's, bit for bit
    triples = sel.select_grasp_points_batch(m, d)
    res_plain = bytes(sel.last_results)
    triples2, cands = sel.select_grasp_candidates_batch(m, d)
    assert bytes(sel.last_results) == res_plain
    assert triples2 == triples
    del m, d
    # (b) every frame equals the single-frame call of its scene
    singles = []
    for s in range(n_scenes):
        t1, c1 = sel.select_grasp_candidates_batch(_dev(masks[s][None]), _dev(depths[s][None]))
        singles.append((t1[0], _valid_rows(c1[0])))
    differ, scored = 0, 0
    for b in range(B):
        rb = _valid_rows(cands[b])
        scored += int(rb["scored"].sum())
        ts, rs = singles[b % n_scenes]
        differ += _assert_frame_equals_single(rb, rs, f"frame {b}")
        if rb["index"][0] == rs["index"][0]:
            assert triples[b] == ts, b
    print(f"headline: {B} frames, {scored} scored candidates, {differ} frames whose order differs at a near-tie")
    assert scored > 0
    # (c) four distinct scenes against the float64 oracle's rows
    for s in (0, 1, 2, 3):
        _, orows = _oracle_rows(P, masks[s], depths[s], True)
        _assert_rows_match_oracle(_valid_rows(cands[s]), orows, f"scene {s}")
        _assert_rows_match_oracle(_valid_rows(cands[B - n_scenes + s]), orows, f"frame {B - n_scenes + s}")


def test_candidate_patches_beyond_one_cnn_slice(sel):
    """416 frames x 20 candidates = 8320 CNN patches: lg_select_grasp's haloed patches run as a slice of 8192 and one of 128.
    uint8 masks: the reference scores border candidates too (replicate padding), so every candidate is scored."""
    H, W = 192, 256
    seeds = (3, 5)
    scenes = [O.synthetic_scene(H, W, s) for s in seeds]
    P = scenes[0][2]
    frames = [(_largest_leaf(lab).astype(np.uint8), dep) for lab, dep, _ in scenes]
    B = 416
    sel.set_camera_params(P)
    masks = np.stack([frames[b % 2][0] for b in range(B)])
    depths = np.stack([frames[b % 2][1] for b in range(B)])
    triples, cands = sel.select_grasp_candidates_batch(_dev(masks), _dev(depths))
    singles = []
    for k in range(2):
        t1, c1 = sel.select_grasp_candidates_batch(_dev(masks[k][None]), _dev(depths[k][None]))
        singles.append((t1[0], _valid_rows(c1[0])))
    scored, differ = 0, 0
    for b in range(B):
        rb = _valid_rows(cands[b])
        scored += int(rb["scored"].sum())
        ts, rs = singles[b % 2]
        differ += _assert_frame_equals_single(rb, rs, f"frame {b}")
        if rb["index"][0] == rs["index"][0]:
            assert triples[b] == ts, b
    print(f"{B} frames at {H}x{W}: {scored} scored candidates, {differ} frames whose order differs at a near-tie")
    assert scored > 8192, scored
    for k in range(2):
        _, orows = _oracle_rows(P, frames[k][0], frames[k][1], True, mask_is_bool=False)
        _assert_rows_match_oracle(_valid_rows(cands[B - 2 + k]), orows, f"seed {seeds[k]}, frame {B - 2 + k}")
