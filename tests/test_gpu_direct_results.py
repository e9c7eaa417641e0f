"""The small results of a call -- every frame's orientation and status word, the near-tile offsets, the result rows -- written by
the kernels straight into the pinned host buffers (device aliases) against the same call with the copies (LG_DIRECT_HOST=0 when
the handle is created): the result rows (last_results) are equal byte for byte and so are the near-tile offsets
(lg_debug_near_tiles), at 96 x 320 and 35 x 130, for batches of 1, 9 and 40 frames with an empty mask among them, and for a
batch of 3 after one of 40 on the same handle.  The same with LG_ORIENT_CAP=16, where a frame with more than 16 runs is handed
back to the host analysis, written into the pinned frame parameters by the host and uploaded."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

SIZES = [(96, 320), (35, 130)]
BATCHES = [40, 3, 1, 9]   # (one handle: 3 after 40)


def _masks(H, W, B):
    """B leaves of different place and size; frame 1 of a batch of more than one is empty"""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        cy, cx = H * (0.3 + 0.05 * (b % 9)), W * (0.15 + 0.08 * (b % 10))
        ry, rx = H * (0.12 + 0.03 * (b % 5)), W * (0.06 + 0.02 * (b % 7))
        out[b] = ((yy - cy) ** 2 / ry ** 2 + (xx - cx) ** 2 / rx ** 2 < 1) & ((xx + 3 * yy + b) % 19 != 0)
    if B > 1:
        out[1] = 0
    return out


@pytest.fixture(scope="module", params=[None, "16"], ids=["device orientation", "LG_ORIENT_CAP=16"])
def handles(request):
    """(direct, copies, cap)"""
    import leafgrasp_amd as L

    assert torch.cuda.is_available()
    keys = ("LG_DIRECT_HOST", "LG_ORIENT_CAP")
    old = {k: os.environ.get(k) for k in keys}
    try:   # the options are read when a handle is created (LG_ORIENT_CAP too: one cap for the handle's life)
        for k in keys:
            os.environ.pop(k, None)
        if request.param:
            os.environ["LG_ORIENT_CAP"] = request.param
        direct = L.GraspPointSelector("cuda:0", load_model=False)
        os.environ["LG_DIRECT_HOST"] = "0"
        copies = L.GraspPointSelector("cuda:0", load_model=False)
        os.environ.pop("LG_DIRECT_HOST")
        yield direct, copies, request.param
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _run(sel, masks, depth):
    from leafgrasp_amd import _lib

    B = masks.shape[0]
    sel.min_edge_distance = 2.0   # small leaves keep valid pixels
    triples = sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), torch.from_numpy(np.stack([depth] * B)).cuda())
    off = (C.c_int32 * (B + 1))()
    assert _lib.lib.lg_debug_near_tiles(sel._h, off, B + 1) == _lib.LG_OK
    redo = C.c_int32(-1)
    assert _lib.lib.lg_debug_orient_redo(sel._h, C.byref(redo)) == _lib.LG_OK
    return triples, bytes(sel.last_results), list(off), redo.value


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_and_offsets_equal_the_copied_ones(handles, size):
    direct, copies, cap = handles
    H, W = size
    _, depth, P = O.synthetic_scene(H, W, seed=4)
    found = handed_back = 0
    for B in BATCHES:
        masks = _masks(H, W, B)
        got = []
        for sel in (direct, copies):
            sel.set_camera_params(P)
            got.append(_run(sel, masks, depth))
        (t_d, rows_d, off_d, redo_d), (t_c, rows_c, off_c, redo_c) = got
        print(f"{size} B={B} cap={cap}: {sum(t[0] is not None for t in t_d)} grasp points, near tiles {off_d[-1]}, handed back {redo_d}")
        assert len(rows_d) == B * 56 and rows_d == rows_c, f"result rows, B={B}"
        assert off_d == off_c and off_d[0] == 0 and off_d[-1] > 0, f"near-tile offsets, B={B}"
        assert all(a <= b for a, b in zip(off_d, off_d[1:]))
        if B > 1:
            assert off_d[1] == off_d[2]          # the empty mask has no near tile
        np.testing.assert_equal(t_d, t_c)
        assert redo_d == redo_c
        found += sum(t[0] is not None for t in t_d)
        handed_back += redo_d
    assert found > 0
    if cap:
        assert handed_back >= 1                  # at least one frame took the host analysis and the upload
    else:
        assert handed_back == 0
