"""Near launch of the score-plane kernel: in sparse mode (lg_select_grasp* called without any plane or validity output)
lg_final_kernel is launched on the tiles around the leaves only (lg_near_tiles), every other tile gets its constant key and
state byte from lg_near_tiles_kernel.  The raw result rows must be bit for bit those of a handle created under LG_FINAL_NEAR=0
(the launch over every tile) and those of the dense call (return_maps=True), and the list offsets the call used
(lg_debug_near_tiles) must be the numpy restatement of the per-tile expression (tests/near_tiles_ref.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import near_tiles_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


def _selector(L, P, monkeypatch=None, **env):
    """a fresh handle; the library reads its switches from the environment when the handle is created"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    for k in env:
        monkeypatch.delenv(k)
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


def _rows(sel, masks, depth, return_maps=False, ip=None):
    """raw result rows of one lg_select_grasp call (bytes of the lg_grasp_result array), and its triples"""
    out = sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), torch.from_numpy(depth).cuda(), return_maps=return_maps,
                                        image_processor=ip)
    torch.cuda.synchronize()
    return bytes(sel.last_results), (out[0] if return_maps else out)


def _near_off(L, sel, B):
    from leafgrasp_amd import _lib

    off = np.full(B + 1, -7, np.int32)
    rc = _lib.lib.lg_debug_near_tiles(sel._h, off.ctypes.data_as(C.POINTER(C.c_int32)), B + 1)
    return rc, off


def _check(L, monkeypatch, masks, depth, P, gaussian_size=5, sel=None, sel0=None):
    """default handle == LG_FINAL_NEAR=0 handle == dense call, byte for byte; the list offsets are the restatement's"""
    from leafgrasp_amd import _lib

    H, W = masks.shape[1:]
    ip = L.ImageProcessor(H, W, 21, gaussian_size)
    sel = sel or _selector(L, P)
    sel0 = sel0 or _selector(L, P, monkeypatch, LG_FINAL_NEAR="0")
    near, triples = _rows(sel, masks, depth, ip=ip)
    rc, off = _near_off(L, sel, len(masks))
    assert rc == 0
    np.testing.assert_array_equal(off, R.near_offsets(masks, gaussian_size // 2 + 1))
    old, _ = _rows(sel0, masks, depth, ip=ip)
    assert _near_off(L, sel0, len(masks))[0] == _lib.LG_ERR_INVALID   # that handle launched every tile
    dense, triples_d = _rows(sel, masks, depth, True, ip=ip)
    assert _near_off(L, sel, len(masks))[0] == _lib.LG_ERR_INVALID    # and so does the dense call
    assert near == old, (triples, "LG_FINAL_NEAR=0")
    assert near == dense, (triples, triples_d)
    assert _rows(sel, masks, depth, ip=ip)[0] == dense                 # and again behind the dense call, on the same handle
    return triples, off


def test_odd_width_partial_tiles_and_the_oracles_grasp_pixel(L, monkeypatch):
    """301 x 517, B = 5: odd width (no 16-byte path), partial last tile row and column"""
    masks, depth, P = _frames(301, 517, [40, 41, 42, 43, 44])
    triples, off = _check(L, monkeypatch, masks, depth, P)
    assert off[-1] > 0
    params = O.cnn_closed_form_params(seed=0)
    for b in (0, 3):
        ref = O.RefGraspPointSelector(cnn=lambda x: O.cnn_forward(params, x))
        ref.set_camera_params(P)
        exp = ref.select_grasp_point(masks[b].astype(np.uint8), depth[b])
        assert triples[b][0] == exp[0], b
        np.testing.assert_allclose(triples[b][1], exp[1], rtol=1e-5)


def test_hand_made_masks_in_one_call(L, monkeypatch):
    """200 x 328 (12.5 tile rows), B = 7: empty, full, single pixels in two corners, a strip along the bottom row, leaves in the
    top-left and bottom-right corners, a leaf in the middle"""
    H, W = 200, 328
    masks, depth, P = _frames(H, W, [7, 8, 9, 10, 11, 12, 13])
    leaf = masks[6].copy()
    masks[:] = False
    masks[1] = True
    masks[2, 0, 0] = masks[2, H - 1, W - 1] = True
    masks[3, H - 1, :] = True
    masks[4, :70, :110] = True
    masks[4, H - 60:, W - 97:] = True
    masks[5, 70:130, 120:230] = True
    masks[6] = leaf
    triples, off = _check(L, monkeypatch, masks, depth, P)
    assert off[1] == 0 and off[2] - off[1] == 6 * 13   # nothing for the empty frame, every tile of the full one
    assert triples[5][0] is not None


@pytest.mark.parametrize("gaussian_size", [1, 3, 5, 7])
def test_mask_edges_step_across_a_tile_boundary(L, monkeypatch, gaussian_size):
    """rectangles whose top and left edges take every offset around the tile boundary y = 48, x = 128 (and their bottom edges
    around y = 64 + ..): the predicate's reach changes with HALO, an off-by-one there turns a leaf tile into a constant one"""
    H, W = 120, 264
    cases = [(y0, x0) for y0 in range(44, 53) for x0 in range(120, 137, 4)]
    _, depth1, P = _frames(H, W, [21])
    depth = np.repeat(depth1, len(cases), axis=0)
    masks = np.zeros((len(cases), H, W), bool)
    for b, (y0, x0) in enumerate(cases):
        masks[b, y0:y0 + 45, x0:x0 + 70] = True
    triples, off = _check(L, monkeypatch, masks, depth, P, gaussian_size)
    assert len(set(np.diff(off).tolist())) > 1        # the steps do change the rectangle
    assert any(t[0] is not None for t in triples)


def test_stale_workspace_on_one_handle(L, monkeypatch):
    """a large leaf, a small leaf elsewhere, a smaller batch, an all-empty batch (nothing is launched): each equal to the same
    call on a fresh handle"""
    H, W = 360, 640
    masks, depth, P = _frames(H, W, [30, 31, 32])
    big = np.zeros_like(masks)
    big[:, 40:330, 60:600] = True
    small = np.zeros_like(masks)
    small[0, 300:340, 20:70] = True
    small[1, 10:50, 560:630] = True
    small[2, 170:200, 300:360] = True
    steps = [big, small, small[:2][::-1].copy(), np.zeros_like(masks)]
    sel = _selector(L, P)
    for i, m in enumerate(steps):
        d = depth[:len(m)]
        got, _ = _rows(sel, m, d)
        rc, off = _near_off(L, sel, len(m))
        assert rc == 0
        np.testing.assert_array_equal(off, R.near_offsets(m, 3))
        fresh, _ = _rows(_selector(L, P), m, d)
        assert got == fresh, i
    assert off[-1] == 0                                # the last step had no near tile at all
    old, _ = _rows(_selector(L, P, monkeypatch, LG_FINAL_NEAR="0"), steps[-1], depth)
    assert got == old


def test_one_frame_and_a_list_length_off_the_xcd_count(L, monkeypatch):
    H, W = 200, 328
    masks, depth, P = _frames(H, W, [50, 51, 52])
    _check(L, monkeypatch, masks[:1], depth[:1], P)
    masks[:] = False
    masks[0, 60:70, 100:110] = True      # 2 x 3 tile rows
    masks[1, 100:101, 10:11] = True      # 1 x 3
    masks[2, 20:30, 200:300] = True      # ...
    _, off = _check(L, monkeypatch, masks, depth, P)
    assert off[-1] % 8 != 0, off


def test_subbatch_pipeline_keeps_the_launch_over_every_tile(L, monkeypatch):
    from leafgrasp_amd import _lib

    masks, depth, P = _frames(200, 328, [60, 61, 62, 63, 64])
    piped = _selector(L, P, monkeypatch, LG_SUBBATCH="2")
    got, _ = _rows(piped, masks, depth)
    assert _near_off(L, piped, 5)[0] == _lib.LG_ERR_INVALID
    want, _ = _rows(_selector(L, P), masks, depth)
    assert got == want


def test_labels_entry_point(L, monkeypatch):
    """select_grasp_points_for_leaves on 4 frames of 360 x 640, one id that no pixel carries"""
    H, W = 360, 640
    scenes = [O.synthetic_scene(H, W, 70 + i) for i in range(4)]
    lab_np = np.stack([s[0] for s in scenes]).astype(np.int16)
    labels = torch.from_numpy(lab_np).cuda()
    depth = torch.from_numpy(np.stack([s[1] for s in scenes])).cuda()
    ids = [_largest_leaf(s[0]) for s in scenes[:3]] + [31000]
    rows = []
    for env in ({}, {"LG_FINAL_NEAR": "0"}):
        sel = _selector(L, scenes[0][2], monkeypatch, **env)
        sel.select_grasp_points_for_leaves(labels, ids, depth)
        torch.cuda.synchronize()
        rows.append(bytes(sel.last_results))
        if not env:
            rc, off = _near_off(L, sel, 4)
            assert rc == 0
            masks = lab_np == np.asarray(ids, np.int16).reshape(-1, 1, 1)
            np.testing.assert_array_equal(off, R.near_offsets(masks, 3))
            assert off[4] == off[3] > 0
    idt = torch.tensor(ids, dtype=torch.int16, device="cuda").reshape(-1, 1, 1)
    sel.select_grasp_points_batch(labels == idt, depth, return_maps=True)
    torch.cuda.synchronize()
    assert rows[0] == rows[1] == bytes(sel.last_results)
