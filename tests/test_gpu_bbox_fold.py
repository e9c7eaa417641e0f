"""The bounding box folded into the bit-row pass (lg_pack_bits16_kernel, lg_pack_bits_kernel, lg_pack_labels16_kernel and the
labels fallback) and lg_window_kernel behind it: every frame's sweep window (dt_maxima(i)[2]), its forms (dt_form(i): searched,
d_out sweeps skipped) and the near-tile offsets (lg_debug_near_tiles, which follow from the box) against numpy, for equality.

Widths: 640 (16 mask bytes per lane), 648 (a multiple of 8 only: one ballot per word) and 130 (not a multiple of 64: the last word
of a row is ragged)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import near_tiles_ref as R  # noqa: E402

A5, B5, C5 = 65536, 91750, 143976      # 16.16 chamfer weights ("Distance transform")
SEARCH_BUDGET = np.float32(2.0e7)      # LG_SEARCH_BUDGET
SHAPES = [(200, 640), (200, 648), (90, 130)]


_SELECTORS = {}


@pytest.fixture
def sel(request):
    """one handle per frame shape: dt_maxima() clips the window it reports to the widest frame its handle has seen"""
    import leafgrasp_amd

    assert torch.cuda.is_available()
    shape = request.getfixturevalue("shape") if "shape" in request.fixturenames else request.node.name
    if shape not in _SELECTORS:
        s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
        s.set_camera_params(O.synthetic_scene(64, 64, 1)[2])
        _SELECTORS[shape] = s
    return _SELECTORS[shape]


def norm5(dx, dy):
    a, b = max(dx, dy), min(dx, dy)
    return (a - 2 * b) * A5 + b * C5 if 2 * b <= a else (a - b) * C5 + (2 * b - a) * B5


def geometry(W):
    """columns per sweep wave, waves per sweep workgroup (lg_dt_geometry)"""
    if W <= 2048:
        return 256, (1 if W <= 256 else 2 if W <= 512 else 4 if W <= 1024 else 8)
    return 512, (8 if W <= 4096 else 16)


def expect(mask):
    """(window, eligible for the row search, d_out sweeps skipped, search cost, box rows) of one frame"""
    H, W = mask.shape
    wc, nw_max = geometry(W)
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return (0, min(W, nw_max * wc), 0, H), False, False, 0, 0
    bx0, bx1, by0, by1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    wx0, wy0 = bx0 // 64 * 64, by0 // 16 * 16
    nw = -(-(bx1 + 1 - wx0) // wc)
    wx1, wy1 = min(W, wx0 + nw * wc), min(H, -(-(by1 + 1) // 16) * 16)
    skip = norm5(max(bx0, W - 1 - bx1), max(by0, H - 1 - by1)) > norm5(wx1 - wx0 - 1, wy1 - wy0 - 1)
    area = int(ys.size)
    a = np.float32(area)
    return (wx0, wx1, wy0, wy1), area < H * W, bool(skip), int(a * np.sqrt(a)), by1 - by0 + 1


def expect_batch(masks):
    """windows, searched, skipped of a batch: the batch is searched while sum of area^1.5 <= budget * rows of its tallest box"""
    e = [expect(np.asarray(m) != 0) for m in masks]
    cost = sum(c for _, el, _, c, _ in e if el)
    rows = max([r for _, el, _, _, r in e if el], default=0)
    sweeps = np.float32(cost) > SEARCH_BUDGET * np.float32(rows)
    return [w for w, *_ in e], [bool(el and not sweeps) for _, el, *_ in e], [s for _, _, s, _, _ in e], cost, rows


def near_off(sel, B):
    from leafgrasp_amd import _lib

    off = np.full(B + 1, -7, np.int32)
    assert _lib.lib.lg_debug_near_tiles(sel._h, off.ctypes.data_as(C.POINTER(C.c_int32)), B + 1) == 0
    return off


def check_last_call(sel, masks, near=True):
    wins, searched, skipped, _, _ = expect_batch(masks)
    B = len(masks)
    assert [sel.dt_maxima(i)[2] for i in range(B)] == wins
    assert [sel.dt_form(i) for i in range(B)] == list(zip(searched, skipped))
    if near:
        np.testing.assert_array_equal(near_off(sel, B), R.near_offsets(np.stack([np.asarray(m) != 0 for m in masks]), 3))


def hand_made(H, W):
    """empty; one pixel in each corner; (W - 1, H - 1) again with a neighbour; a full frame; a leaf on each border; values > 1"""
    m = np.zeros((12, H, W), np.uint8)
    m[1, 0, 0] = m[2, 0, W - 1] = m[3, H - 1, 0] = m[4, H - 1, W - 1] = 1
    m[5, H - 1, W - 1] = m[5, H - 2, W - 2] = 1
    m[6] = 1
    m[7, :H // 3, W // 3:W // 2] = 1          # top
    m[8, H // 2:, W // 4:W // 2] = 1          # bottom
    m[9, H // 4:H // 2, :W // 5] = 1          # left
    m[10, H // 3:H // 2 + 5, W - W // 3:] = 1  # right
    m[11, H // 3:H // 2, W // 3:W // 2 + 3] = np.arange(2, 2 + W // 2 + 3 - W // 3, dtype=np.uint8)[None, :] | 2
    return m


def depth_for(B, H, W):
    return torch.from_numpy(np.broadcast_to(O.synthetic_scene(H, W, 2)[1], (B, H, W)).copy()).cuda()


@pytest.mark.parametrize("shape", SHAPES)
def test_one_frame_at_a_time(sel, shape):
    H, W = shape
    masks = hand_made(H, W)
    d = depth_for(1, H, W)
    for b in range(len(masks)):
        sel.select_grasp_points_batch(torch.from_numpy(masks[b:b + 1]).cuda(), d)
        check_last_call(sel, masks[b:b + 1])


@pytest.mark.parametrize("as_bool", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_nine_mixed_frames(sel, shape, as_bool):
    H, W = shape
    masks = hand_made(H, W)[[0, 4, 6, 7, 1, 11, 10, 8, 5]]
    m = torch.from_numpy(masks != 0 if as_bool else masks).cuda()
    sel.select_grasp_points_batch(m, depth_for(9, H, W))
    check_last_call(sel, masks)


def test_misaligned_mask_takes_the_ballot_kernel(sel):
    H, W = 200, 640
    masks = hand_made(H, W)[[7, 0, 5]]
    buf = torch.zeros(3 * H * W + 16, dtype=torch.uint8, device="cuda")
    m = buf[3:3 + 3 * H * W].view(3, H, W)
    m.copy_(torch.from_numpy(masks))
    assert m.data_ptr() % 16 != 0
    sel.select_grasp_points_batch(m, depth_for(3, H, W))
    check_last_call(sel, masks)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_labels_entry(sel, shape, misaligned):
    H, W = shape
    masks = hand_made(H, W)[[8, 0, 2, 6, 9]] != 0
    rng = np.random.default_rng(4)
    ids = [3, 5, 7, 2, 9]
    labels = rng.integers(10, 20, (5, H, W)).astype(np.int16)        # other leaves everywhere else
    for b in range(5):
        labels[b][masks[b]] = ids[b]
    buf = torch.zeros(5 * H * W + 8, dtype=torch.int16, device="cuda")
    lab = buf[1:1 + 5 * H * W].view(5, H, W) if misaligned else buf[:5 * H * W].view(5, H, W)
    lab.copy_(torch.from_numpy(labels))
    assert (lab.data_ptr() % 16 != 0) == misaligned
    sel.select_grasp_points_for_leaves(lab, ids, depth_for(5, H, W))
    check_last_call(sel, masks)


def test_search_or_sweeps_on_each_side_of_the_budget(sel):
    """frames with one zero pixel, 200 x 640: 87 of them cost 3.98e9 <= 2e7 * 200 rows and are searched, 88 cost 4.03e9 and are
    swept; an empty and a full frame in the batch add nothing to either sum"""
    H, W = 200, 640
    one = np.ones((H, W), np.uint8)
    one[77, 301] = 0
    for n, want in ((87, True), (88, False)):
        masks = np.concatenate([np.zeros((1, H, W), np.uint8), np.ones((1, H, W), np.uint8), np.repeat(one[None], n, 0)])
        _, searched, _, cost, rows = expect_batch(masks)
        assert rows == 200 and (np.float32(cost) <= SEARCH_BUDGET * np.float32(rows)) == want
        assert searched == [False, False] + [want] * n
        sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), depth_for(len(masks), H, W))
        check_last_call(sel, masks)


def test_more_frames_than_the_window_kernel_has_threads(sel):
    H, W = 48, 130
    base = hand_made(H, W)
    masks = base[np.arange(1100) % len(base)]
    sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), depth_for(len(masks), H, W))
    check_last_call(sel, masks)
