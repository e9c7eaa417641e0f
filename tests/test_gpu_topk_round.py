"""The greedy spaced top-k on the device (lg_topk_kernel through lg_topk_nms and through lg_select_grasp_candidates) against the
walk it implements, restated in numpy: repeat { arg-max over the pixels still alive (score descending, flat index descending);
kill the Chebyshev ball of radius 2 * min_distance around the pick }.  tests/test_properties.py holds that formulation against
the reference's walk over the full argsort; here it is the reference, and every comparison is for equality.

The shapes pick the kernel's forms: 48 x 128 (W % 4 == 0: a wave per touched tile), 50 x 130 (the general form; a ragged last tile
row and column), 16 x 64 (one tile), 2160 x 3840 (8100 tiles, several per thread in the arg-max over the tile keys); min_distance
40 makes a window touch more than eight tiles, which takes the general form at any width."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

SMALL = [(48, 128), (50, 130), (16, 64)]
BIG = (2160, 3840)


@pytest.fixture(scope="module")
def sel():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)


def greedy(trad, valid, k, md):
    """[(x, y)] of one frame: the iterative masked arg-max over trad * valid (a product, as the reference's valid_scores)."""
    H, W = trad.shape
    flat = (trad * valid.astype(np.float32) + np.float32(0.0)).ravel()
    alive = np.ones((H, W), bool)
    out = []
    for _ in range(k):
        a = alive.ravel()
        if not a.any():
            break
        m = flat[a].max()
        idx = int(np.flatnonzero(a & (flat == m))[-1])   # a tie goes to the higher flat index
        y, x = divmod(idx, W)
        out.append((x, y))
        alive[max(0, y - 2 * md):y + 2 * md + 1, max(0, x - 2 * md):x + 2 * md + 1] = False
    return out


def device(sel, trad, valid, k, md):
    """[[(x, y)]] of every frame, from out_xy[:out_n] of lg_topk_nms"""
    res = sel._get_candidate_points(torch.from_numpy(trad).cuda(), torch.from_numpy(valid.astype(np.uint8)).cuda(), k, md)
    return [res] if trad.shape[0] == 1 else res


def check(sel, trad, valid, k, md):
    trad = np.ascontiguousarray(trad, np.float32)
    valid = np.ascontiguousarray(valid)
    got = device(sel, trad, valid, k, md)
    assert len(got) == trad.shape[0]
    for b in range(trad.shape[0]):
        assert got[b] == greedy(trad[b], valid[b], k, md), (b, trad.shape, k, md)
    return got


def frames(shape, B, seed):
    """B different frames: smooth random scores, rounded ones (ties), and negative ones under a sparse validity plane"""
    H, W = shape
    rng = np.random.default_rng(seed)
    trad = rng.random((B, H, W)).astype(np.float32)
    valid = rng.random((B, H, W)) > 0.3
    if B > 1:
        trad[1] = np.round(trad[1], 1)
    if B > 2:
        trad[2] -= np.float32(0.7)
        valid[2] = rng.random((H, W)) > 0.9
    return trad, valid


@pytest.mark.parametrize("md", [0, 10, 40])
@pytest.mark.parametrize("k", [1, 20, 64])
@pytest.mark.parametrize("shape", SMALL)
def test_three_different_frames(sel, shape, k, md):
    trad, valid = frames(shape, 3, seed=shape[0] * 100 + k + md)
    got = check(sel, trad, valid, k, md)
    if md == 0:
        assert all(len(g) == k for g in got)          # nothing but the pick itself is suppressed
    if md >= 10 and k == 64:
        assert all(len(g) < k for g in got)           # picks lie more than 20 apart: at most 7 x 3 fit, the walk ends early


@pytest.mark.parametrize("md", [0, 10, 40])
def test_one_4k_frame(sel, md):
    trad, valid = frames(BIG, 1, seed=7 + md)
    got = check(sel, trad, valid, 20, md)
    assert len(got[0]) == 20


@pytest.mark.parametrize("shape", SMALL)
def test_fewer_valid_pixels_than_k(sel, shape):
    H, W = shape
    rng = np.random.default_rng(3)
    trad = rng.random((3, H, W)).astype(np.float32) + np.float32(0.25)
    valid = np.zeros((3, H, W), bool)
    for b, npx in enumerate((5, 1, 0)):
        valid.reshape(3, -1)[b, rng.choice(H * W, npx, replace=False)] = True
    for md in (0, 10):
        got = check(sel, trad, valid, 64, md)
        if md == 10:
            assert all(len(g) < 64 for g in got)      # (an invalid pixel scores 0 and is still picked: only suppression ends the walk)


@pytest.mark.parametrize("md", [0, 3, 10])
@pytest.mark.parametrize("shape", SMALL)
def test_constant_plateau_ties_go_to_the_higher_flat_index(sel, shape, md):
    H, W = shape
    trad = np.full((1, H, W), 0.5, np.float32)
    got = check(sel, trad, np.ones((1, H, W), bool), 20, md)
    assert got[0][0] == (W - 1, H - 1)


@pytest.mark.parametrize("md", [3, 10, 40])
@pytest.mark.parametrize("shape", SMALL + [BIG])
def test_maxima_in_the_four_corners(sel, shape, md):
    H, W = shape
    rng = np.random.default_rng(11)
    trad = (rng.random((1, H, W)) * 0.5).astype(np.float32)
    for i, (y, x) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]):
        trad[0, y, x] = 1.0 + 0.1 * i
    got = check(sel, trad, np.ones((1, H, W), bool), 8, md)
    assert got[0][0] == (W - 1, H - 1)


PAIRS = [  # (md, first peak (x, y), axis): the second peak lies 2 md and 2 md + 1 further along the axis
    (10, (5, 4), "x"),     # both inside tile column 0
    (10, (54, 4), "x"),    # across the boundary between tile columns 0 and 1
    (3, (10, 2), "y"),     # both inside tile row 0
    (3, (10, 12), "y"),    # across the boundary between tile rows 0 and 1
    (3, (61, 9), "x"),     # across the column boundary, a small window
]


@pytest.mark.parametrize("md,p0,axis", PAIRS)
@pytest.mark.parametrize("shape", [(48, 128), (50, 130)])
def test_two_maxima_at_the_edge_of_a_window(sel, shape, md, p0, axis):
    H, W = shape
    rng = np.random.default_rng(5)
    base = (rng.random((H, W)) * 0.5).astype(np.float32)
    trad = np.stack([base, base])
    x0, y0 = p0
    for b, d in enumerate((2 * md, 2 * md + 1)):
        x1, y1 = (x0 + d, y0) if axis == "x" else (x0, y0 + d)
        trad[b, y0, x0] = 1.0
        trad[b, y1, x1] = 0.9
    got = check(sel, trad, np.ones((2, H, W), bool), 4, md)
    d0 = (x0 + 2 * md, y0) if axis == "x" else (x0, y0 + 2 * md)
    d1 = (x0 + 2 * md + 1, y0) if axis == "x" else (x0, y0 + 2 * md + 1)
    assert got[0][0] == p0 and d0 not in got[0]        # exactly 2 md away: inside the window, suppressed
    assert got[1][:2] == [p0, d1]                        # one further: the second pick


def test_the_selection_call_walks_the_same_candidates(sel):
    """lg_select_grasp_candidates (sparse planes: tile keys and tile states from the plane kernel) against the oracle's walk on
    the planes lg_score_maps writes"""
    Hs, Ws = 360, 640
    masks, depths = [], []
    for seed in (3, 8):
        labels, depth, P = O.synthetic_scene(Hs, Ws, seed)
        ids, counts = np.unique(labels[labels > 0], return_counts=True)
        masks.append(labels == int(ids[np.argmax(counts)]))
        depths.append(depth)
    sel.set_camera_params(P)
    sel.clear_cnn()
    m = torch.from_numpy(np.stack(masks)).cuda()
    d = torch.from_numpy(np.stack(depths).astype(np.float32)).cuda()
    _, cands = sel.select_grasp_candidates_batch(m, d, top_k=20)
    maps, valid, _ = sel.score_maps(m.to(torch.uint8), d)
    trad, valid = maps["traditional_score"].cpu().numpy(), valid.cpu().numpy() != 0
    ref = O.RefGraspPointSelector()
    for b in range(2):
        rows = cands[b][cands[b]["index"] >= 0]
        rows = rows[np.argsort(rows["index"])]
        got = [(int(r["x"]), int(r["y"])) for r in rows]
        want = ref._get_candidate_points(trad[b], valid[b], 20, 10)
        assert got == want and len(got) > 1, b
