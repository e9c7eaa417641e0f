"""The sweep window from the five words the bit-row pass accumulates (lg_window_from_box: the code lg_window_kernel runs),
without a device.  The words all start from zero, so the two minima of the bounding box are held as maxima (W - 1 - x0,
H - 1 - y0) and an area of zero means an empty mask; the window, the forms and the decoded box must be those of a numpy
restatement on the mask itself, and the decoded box must give lg_near_tile_rect the rectangle the mask's own box gives."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402
from tests import near_tiles_ref as R  # noqa: E402

A5, B5, C5 = 65536, 91750, 143976
SHAPES = [(40, 130), (88, 200), (33, 64), (200, 648), (60, 2100)]


def norm5(dx, dy):
    a, b = max(dx, dy), min(dx, dy)
    return (a - 2 * b) * A5 + b * C5 if 2 * b <= a else (a - b) * C5 + (2 * b - a) * B5


def encode(mask):
    """what the pack kernels leave behind: maxima and a sum over the set pixels, every word starting from 0"""
    H, W = mask.shape
    box = np.zeros(5, np.uint32)
    for y, x in zip(*np.nonzero(mask)):
        box[0] = max(box[0], W - 1 - x)
        box[1] = max(box[1], x)
        box[2] = max(box[2], H - 1 - y)
        box[3] = max(box[3], y)
        box[4] += 1
    return box


def lib_window(box, H, W, mode):
    out = (C.c_int32 * 12)()
    rc = _lib.lib.lg_window_from_box(box.ctypes.data_as(C.POINTER(C.c_uint32)), H, W, mode, out)
    assert rc == 0
    return list(out)


def expect(mask, mode):
    H, W = mask.shape
    wc = 256 if W <= 2048 else 512
    nw_max = (1 if W <= 256 else 2 if W <= 512 else 4 if W <= 1024 else 8) if W <= 2048 else (8 if W <= 4096 else 16)
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return [0, min(W, nw_max * wc), 0, H, 0, -1, 0, -1, 0, 0, 0, wc]
    bx0, bx1, by0, by1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    wx0, wy0 = bx0 // 64 * 64, by0 // 16 * 16
    wx1 = min(W, wx0 + -(-(bx1 + 1 - wx0) // wc) * wc)
    wy1 = min(H, -(-(by1 + 1) // 16) * 16)
    skip = norm5(max(bx0, W - 1 - bx1), max(by0, H - 1 - by1)) > norm5(wx1 - wx0 - 1, wy1 - wy0 - 1)
    return [wx0, wx1, wy0, wy1, bx0, bx1, by0, by1, int(skip), int(mode != 0 and ys.size < H * W), int(ys.size), wc]


def masks_of(H, W, rng):
    yield np.zeros((H, W), bool)
    yield np.ones((H, W), bool)
    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        m = np.zeros((H, W), bool)
        m[y, x] = True
        yield m
    for _ in range(30):
        y0, y1 = sorted(rng.integers(0, H, 2))
        x0, x1 = sorted(rng.integers(0, W, 2))
        m = np.zeros((H, W), bool)
        m[y0:y1 + 1, x0:x1 + 1] = rng.random((y1 - y0 + 1, x1 - x0 + 1)) < 0.2
        m[y0, rng.integers(x0, x1 + 1)] = m[y1, rng.integers(x0, x1 + 1)] = True
        m[rng.integers(y0, y1 + 1), x0] = m[rng.integers(y0, y1 + 1), x1] = True
        yield m


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_window_forms_and_decoded_box(shape, mode):
    H, W = shape
    rng = np.random.default_rng(H * 7 + W + mode)
    for m in masks_of(H, W, rng):
        got = lib_window(encode(m), H, W, mode)
        assert got == expect(m, mode)
        wx0, wx1, wy0, wy1, bx0, bx1, by0, by1 = got[:8]
        assert wx0 % 64 == 0 and wy0 % 16 == 0 and (wy1 % 16 == 0 or wy1 == H)
        if m.any():   # the window holds the box
            assert wx0 <= bx0 and bx1 < wx1 and wy0 <= by0 and by1 < wy1


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_the_decoded_box_gives_the_masks_near_tiles(shape):
    H, W = shape
    rng = np.random.default_rng(W)
    rect = (C.c_int32 * 4)()
    for m in masks_of(H, W, rng):
        got = lib_window(encode(m), H, W, 2)
        for halo in (1, 3):
            n = _lib.lib.lg_near_tile_rect(got[4], got[5], got[6], got[7], H, W, halo, rect)
            assert (tuple(rect), n) == R.rect_of(R.near_map(R.bbox(m), H, W, halo))


def test_the_other_four_words_do_not_matter_when_the_area_is_zero():
    want = lib_window(np.zeros(5, np.uint32), 90, 130, 2)
    assert lib_window(np.array([7, 100, 3, 60, 0], np.uint32), 90, 130, 2) == want
    assert want[4:8] == [0, -1, 0, -1] and want[8:11] == [0, 0, 0]


def test_bad_arguments():
    out = (C.c_int32 * 12)()
    box = np.array([0, 0, 0, 0, 1], np.uint32)
    p = box.ctypes.data_as(C.POINTER(C.c_uint32))
    fn = _lib.lib.lg_window_from_box
    assert fn(p, 64, 64, 2, out) == 0
    assert fn(None, 64, 64, 2, out) == _lib.LG_ERR_INVALID
    assert fn(p, 64, 64, 2, None) == _lib.LG_ERR_INVALID
    assert fn(p, 0, 64, 2, out) == _lib.LG_ERR_INVALID
    assert fn(p, 64, 9000, 2, out) == _lib.LG_ERR_INVALID
    assert fn(p, 64, 64, 3, out) == _lib.LG_ERR_INVALID
    box[1] = 64   # a column past the frame
    assert fn(p, 64, 64, 2, out) == _lib.LG_ERR_INVALID
