"""lg_select_grasp with the CNN on the candidates that can still win only (the default) against a handle created with
LG_CNN_PRUNE=0 (every candidate's patch through the CNN): the result rows are equal byte for byte, a repeated call equals
itself, and lg_debug_cnn_scored is exactly the number the exported predicate (lg_cnn_candidate_cannot_win) and the border
rule give on the rows of select_grasp_candidates_batch for the same frames -- a build whose pruning is silently off fails."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

WEIGHTS = ("w_approach", "w_sdf", "w_flat", "w_access")


def _selector(params):
    import leafgrasp_amd

    s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    s.set_cnn_state_dict(params)
    return s


@pytest.fixture(scope="module")
def pair():
    """(default handle, handle created with LG_CNN_PRUNE=0): the switch is read at lg_create."""
    assert torch.cuda.is_available()
    mp = pytest.MonkeyPatch()
    mp.delenv("LG_CNN_PRUNE", raising=False)
    on = _selector(O.cnn_closed_form_params(seed=0))
    mp.setenv("LG_CNN_PRUNE", "0")
    off = _selector(O.cnn_closed_form_params(seed=0))
    mp.undo()
    yield on, off
    on.clear_cnn()
    off.clear_cnn()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _largest_leaf(labels):
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    return labels == ids[np.argmax(counts)]


@functools.lru_cache(maxsize=None)
def _small(H, W, seeds):
    scenes = [O.synthetic_scene(H, W, s) for s in seeds]
    masks = np.stack([_largest_leaf(lab) for lab, _, _ in scenes])
    depths = np.stack([dep for _, dep, _ in scenes])
    return masks, depths, scenes[0][2]


def _expected_scored(cands, H, W, is_bool):
    """Patches the pruned call must put through the CNN, from the candidates entry's rows: a frame with more than one
    candidate; of its candidates those the rescoring scores (border rule of a torch.bool mask) that can still beat candidate
    0's traditional score."""
    import leafgrasp_amd as L

    total, eligible = 0, 0
    for rows in cands:
        rows = rows[rows["index"] >= 0]
        if len(rows) <= 1:
            assert not rows["scored"].any()
            continue
        t0 = float(rows["traditional"][rows["index"] == 0][0])
        for r in rows:
            x, y = int(r["x"]), int(r["y"])
            border = is_bool and (x < 16 or y < 16 or x + 16 > W or y + 16 > H)
            assert bool(r["scored"]) == (not border)
            if border:
                continue
            eligible += 1
            total += 0 if L._lib.lib.lg_cnn_candidate_cannot_win(float(r["traditional"]), t0) else 1
    return total, eligible


def _check(pair, masks, depths, P, what, top_k=20):
    """-> (patches scored with pruning, eligible candidates, B * top_k)."""
    on, off = pair
    m, d = _dev(masks), _dev(depths)
    B, H, W = masks.shape
    is_bool = masks.dtype == np.bool_
    got = {}
    for name, s in (("pruned", on), ("all", off)):
        s.set_camera_params(P)
        s.params.top_k = top_k
        try:
            t1 = s.select_grasp_points_batch(m, d)
            r1 = bytes(s.last_results)
            n1 = s.cnn_scored()
            t2 = s.select_grasp_points_batch(m, d)
            assert bytes(s.last_results) == r1 and t2 == t1, f"{what}: {name}, repeated call"
            assert s.cnn_scored() == n1
        finally:
            s.params.top_k = 20
        got[name] = (t1, r1, n1)
    assert got["pruned"][1] == got["all"][1], f"{what}: result rows with and without pruning"
    assert got["pruned"][0] == got["all"][0]
    assert got["all"][2] == B * top_k, what
    # the candidates entry scores every candidate and returns the same result rows
    for s in (on, off):
        _, cands = s.select_grasp_candidates_batch(m, d, top_k=top_k)
        assert bytes(s.last_results) == got["pruned"][1], f"{what}: candidates entry"
        assert s.cnn_scored() == B * top_k
    expected, eligible = _expected_scored(cands, H, W, is_bool)
    print(f"{what}: {got['pruned'][2]} of {B * top_k} patches through the CNN ({eligible} eligible candidates)")
    assert got["pruned"][2] == expected, (what, got["pruned"][2], expected)
    return expected, eligible, B * top_k


def test_benchmark_scenes_1080p(pair):
    import bench

    masks, depths, P, _ = bench.make_frames(32, 1080, 1920, workers=1)
    assert masks.dtype == np.bool_ and masks.shape[0] == 32
    scored, eligible, total = _check(pair, masks, depths, P, "32 benchmark scenes")
    assert total == 640
    assert 0 < scored <= 0.25 * total, scored     # the float64 oracle's rows give 115 (18.0 %)


@pytest.mark.parametrize("as_bool", [True, False], ids=["bool", "uint8"])
def test_small_scenes(pair, as_bool):
    """uint8 masks: border candidates are scored (replicate padding); bool masks: they are not."""
    masks, depths, P = _small(384, 512, (3, 4, 6, 9))
    m = masks if as_bool else masks.astype(np.uint8)
    scored, eligible, total = _check(pair, m, depths, P, f"384x512 {'bool' if as_bool else 'uint8'}")
    assert scored <= eligible
    if not as_bool:   # every candidate is eligible, and candidate 0 of a frame can always be lifted above its own score
        assert eligible > 0 and scored > 0


@pytest.mark.parametrize("top_k", [1, 2, 5, 20, 64])
def test_top_k(pair, top_k):
    masks, depths, P = _small(384, 512, (3, 4))
    scored, eligible, total = _check(pair, masks, depths, P, f"top_k {top_k}", top_k=top_k)
    if top_k == 1:
        assert scored == 0      # a frame with one candidate is not rescored


def test_empty_mask(pair):
    """An empty mask still has candidates (score * valid is 0 everywhere: the walk takes the last pixels of the frame, all
    with the constant tile's traditional score), so whatever of them lies off the border survives."""
    masks, depths, P = _small(384, 512, (3, 4))
    m = masks.copy()
    m[1] = False
    _check(pair, m, depths, P, "one empty mask")
    m[:] = False
    _check(pair, m, depths, P, "all masks empty")
    _check(pair, m.astype(np.uint8), depths, P, "all masks empty, uint8")


def test_more_than_one_cnn_slice(pair):
    """416 frames x 20 candidates = 8320 patch slots (uint8 masks: every candidate is eligible): the unpruned pass runs a slice
    of 8192 and one of 128; the pruned one takes its count from the device in both."""
    masks, depths, P = _small(192, 256, (3, 5))
    B = 416
    m = np.stack([masks[b % 2] for b in range(B)]).astype(np.uint8)
    d = np.stack([depths[b % 2] for b in range(B)])
    scored, eligible, total = _check(pair, m, d, P, "416 frames of 192x256")
    assert total == 8320 and 0 < scored <= eligible


def test_low_scores(pair):
    """The four score weights halved: traditional scores below 0.5, where a candidate within 0.225 of the best survives (the
    candidates the walk takes off the valid region, with traditional score 0, still do not)."""
    masks, depths, P = _small(384, 512, (3, 4, 6, 9))
    on, off = pair
    keep = {w: getattr(on.params, w) for w in WEIGHTS}
    try:
        for s in pair:
            for w in WEIGHTS:
                setattr(s.params, w, keep[w] * 0.5)
        m8 = masks.astype(np.uint8)
        scored, eligible, total = _check(pair, m8, depths, P, "halved weights")
    finally:
        for s in pair:
            for w in WEIGHTS:
                setattr(s.params, w, keep[w])
    assert eligible > 0 and scored > 0, (scored, eligible)   # (how many survive is checked exactly, in _check)


@pytest.mark.parametrize("name", ["wide_range", "hybrid"])
def test_other_weights(pair, name):
    from tests.test_gpu_parity import _wide_range_params

    params = _wide_range_params(0) if name == "wide_range" else O.cnn_closed_form_params(seed=1, attention_type="hybrid")
    masks, depths, P = _small(384, 512, (3, 4, 6, 9))
    try:
        for s in pair:
            s.set_cnn_state_dict(params)
        _check(pair, masks, depths, P, name)
        _check(pair, masks.astype(np.uint8), depths, P, name + " uint8")
    finally:
        for s in pair:
            s.set_cnn_state_dict(O.cnn_closed_form_params(seed=0))
