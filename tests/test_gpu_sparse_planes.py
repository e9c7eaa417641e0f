"""Sparse planes: lg_select_grasp / lg_select_grasp_labels called without any plane or validity output leave the constant tiles of
their workspace planes unwritten (lg_final_kernel records per tile which it wrote; top-k and the patch gather substitute the
constant tile's values).  The result rows -- point, 3-D points, best_score, ml_used, n_candidates, theta -- must be bit for bit
those of the same call with every plane written (return_maps=True), on the same handle and inputs, with the CNN loaded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


def _selector(L, P):
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_camera_params(P)
    sel.set_cnn_state_dict(O.cnn_closed_form_params(seed=0))
    return sel


def _largest_leaf(labels):
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    return int(ids[np.argmax(counts)])


def _frames(H, W, seeds):
    scenes = [O.synthetic_scene(H, W, s) for s in seeds]
    masks = np.stack([(lab == _largest_leaf(lab)) for lab, _, _ in scenes])
    depth = np.stack([d for _, d, _ in scenes])
    return masks, depth, scenes[0][2]


def _rows(sel, masks, depth, return_maps):
    """raw result rows of one lg_select_grasp call (bytes of the lg_grasp_result array)"""
    out = sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), torch.from_numpy(depth).cuda(), return_maps=return_maps)
    torch.cuda.synchronize()
    return bytes(sel.last_results), (out[0] if return_maps else out)


def _assert_sparse_equals_dense(sel, masks, depth):
    sparse, triples = _rows(sel, masks, depth, False)
    dense, triples_d = _rows(sel, masks, depth, True)
    assert sparse == dense, (triples, triples_d)
    # and in the other order on the same handle: the dense call's planes do not help the sparse one
    assert _rows(sel, masks, depth, False)[0] == dense
    return triples


def test_sparse_rows_equal_dense_1080p_b32(L):
    masks, depth, P = _frames(1080, 1920, range(100, 132))
    sel = _selector(L, P)
    triples = _assert_sparse_equals_dense(sel, masks, depth)
    assert all(t[0] is not None for t in triples)


@pytest.mark.parametrize("shape", [(301, 517), (2160, 3840)])
def test_sparse_rows_equal_dense_odd_width_and_4k(L, shape):
    H, W = shape
    masks, depth, P = _frames(H, W, [40, 41, 42, 43] if H < 1000 else [40, 41])
    _assert_sparse_equals_dense(_selector(L, P), masks, depth)


def test_sparse_rows_equal_dense_empty_mask_and_border_leaf(L):
    H, W = 360, 640
    masks, depth, P = _frames(H, W, [7, 8, 9, 10])
    masks[0] = False                                     # empty mask: every tile constant, the fall-through picks
    masks[1] = False
    masks[1, :90, :150] = True                           # a leaf in the top-left corner, touching two frame borders
    masks[2] = False
    masks[2, H - 70:, W - 133:] = True                   # ... in the bottom-right corner
    masks[3, :, :5] = True                               # a strip down the left border next to the leaf
    _assert_sparse_equals_dense(_selector(L, P), masks, depth)


def test_sparse_rows_equal_dense_fewer_valid_pixels_than_top_k(L):
    H, W = 256, 384
    masks, depth, P = _frames(H, W, [11, 12, 13])
    for b, (y, x, r) in enumerate([(100, 200, 3), (30, 40, 7), (200, 350, 9)]):
        masks[b] = False
        masks[b, y - r:y + r + 1, x - r:x + r + 1] = True   # a small square: a few valid pixels at most, picks on constant tiles
    sel = _selector(L, P)
    triples = _assert_sparse_equals_dense(sel, masks, depth)
    assert any(t[0] is not None for t in triples)


def test_sparse_rows_equal_dense_general_topk_path(L):
    masks, depth, P = _frames(540, 960, [14, 15, 16])
    sel = _selector(L, P)
    sel.params.nms_min_distance = 40   # an 161 x 161 suppression window touches more than 8 tiles: the general top-k form
    _assert_sparse_equals_dense(sel, masks, depth)
    sel.params.top_k = 64
    sel.params.nms_min_distance = 25
    _assert_sparse_equals_dense(sel, masks, depth)


def test_sparse_labels_entry_point_equals_dense_masks_path(L):
    H, W = 720, 1280
    scenes = [O.synthetic_scene(H, W, 60 + i) for i in range(4)]
    labels = torch.from_numpy(np.stack([s[0] for s in scenes]).astype(np.int16)).cuda()
    depth = torch.from_numpy(np.stack([s[1] for s in scenes])).cuda()
    ids = [_largest_leaf(s[0]) for s in scenes[:3]] + [31000]   # (an id no pixel carries: an empty mask)
    sel = _selector(L, scenes[0][2])
    got = sel.select_grasp_points_for_leaves(labels, ids, depth)
    torch.cuda.synchronize()
    rows = bytes(sel.last_results)
    idt = torch.tensor(ids, dtype=torch.int16, device="cuda").reshape(-1, 1, 1)
    want, _, _ = sel.select_grasp_points_batch(labels == idt, depth, return_maps=True)
    torch.cuda.synchronize()
    assert rows == bytes(sel.last_results), (got, want)


def test_sparse_stale_workspace(L):
    """Scene A, then a scene B whose leaf lies elsewhere, on one handle: the tiles A materialised hold A's planes, which B's call
    must not read.  Equal to B on a fresh handle, and to B with every plane written."""
    H, W = 540, 960
    masks_a, depth_a, P = _frames(H, W, [17, 18])
    masks_b = np.zeros_like(masks_a)
    masks_b[0, 300:420, 600:800] = True               # B's leaves away from A's
    masks_b[1, 20:120, 30:230] = True
    masks_b[1] &= ~masks_a[1]
    depth_b = depth_a[::-1].copy()
    sel = _selector(L, P)
    _rows(sel, masks_a, depth_a, True)                 # every plane of A written
    _rows(sel, masks_a, depth_a, False)
    stale, _ = _rows(sel, masks_b, depth_b, False)
    fresh, _ = _rows(_selector(L, P), masks_b, depth_b, False)
    dense, _ = _rows(_selector(L, P), masks_b, depth_b, True)
    assert stale == fresh == dense
