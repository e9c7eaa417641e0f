"""The rectangle of near tiles (lg_near_tile_rect: the code lg_final_kernel and the enumeration kernel run), without a device:
equal to the per-tile expression restated in numpy (tests/near_tiles_ref.py) for every bounding box on a grid of corners, and
-- the property that matters -- every tile whose bit-row test can find a mask bit lies inside it."""
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

SHAPES = [(40, 130), (88, 200), (33, 64)]
HALOS = [1, 2, 3, 4]


def lib_rect(box, H, W, halo):
    rect = (C.c_int32 * 4)()
    n = _lib.lib.lg_near_tile_rect(box[0], box[1], box[2], box[3], H, W, halo, rect)
    return tuple(rect), n


def corners(n, tile, halo):
    """0, n-1 and, around every tile boundary b: b, b-1, b +- (halo-1, halo, halo+1) (the row test's reach ends there), b +- (7,
    8, 9) (the column test's)"""
    v = {0, n - 1}
    for b in range(tile, n + tile, tile):
        for d in (0, -1, halo - 1, halo, halo + 1, -(halo - 1), -halo, -(halo + 1), 7, 8, 9, -7, -8, -9):
            v.add(b + d)
    return sorted(x for x in v if 0 <= x < n)


@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("shape", SHAPES)
def test_rectangle_equals_the_per_tile_expression_on_a_grid_of_boxes(shape, halo):
    H, W = shape
    xs, ys = corners(W, R.TW, halo), corners(H, R.TH, halo)
    colh, rowh = R.near_map_grid(xs, ys, H, W, halo)   # [i, j, tx], [k, l, ty]
    rect = (C.c_int32 * 4)()
    fn = _lib.lib.lg_near_tile_rect

    def span(v):   # (lo, hi) of a 1-D bool vector that must be one run
        idx = np.nonzero(v)[0]
        if idx.size == 0:
            return None
        assert idx[-1] - idx[0] + 1 == idx.size
        return int(idx[0]), int(idx[-1])

    xspan = {(i, j): span(colh[i, j]) for i in range(len(xs)) for j in range(i, len(xs))}
    yspan = {(k, l): span(rowh[k, l]) for k in range(len(ys)) for l in range(k, len(ys))}
    n_boxes = 0
    for (i, j), sx in xspan.items():
        for (k, l), sy in yspan.items():
            n = fn(xs[i], xs[j], ys[k], ys[l], H, W, halo, rect)
            if sx is None or sy is None:
                want, cnt = (0, -1, 0, -1), 0
            else:
                want, cnt = (sx[0], sx[1], sy[0], sy[1]), (sx[1] - sx[0] + 1) * (sy[1] - sy[0] + 1)
            assert (tuple(rect), n) == (want, cnt), (xs[i], xs[j], ys[k], ys[l])
            n_boxes += 1
    assert n_boxes >= 1000
    # a sample of them against the tile-by-tile loop itself (the vectorised form above is the same expression)
    rng = np.random.default_rng(halo * 1000 + H)
    for _ in range(40):
        i, j = sorted(rng.integers(0, len(xs), 2))
        k, l = sorted(rng.integers(0, len(ys), 2))
        box = (xs[i], xs[j], ys[k], ys[l])
        assert lib_rect(box, H, W, halo) == R.rect_of(R.near_map(box, H, W, halo)), box


@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("shape", SHAPES)
def test_empty_and_inverted_boxes_have_no_near_tile(shape, halo):
    H, W = shape
    for box in [(0, -1, 0, -1), (5, 4, 3, 20), (W - 1, 0, 0, H - 1), (10, 9, 12, 11)]:
        assert lib_rect(box, H, W, halo) == ((0, -1, 0, -1), 0)
        assert not R.near_map(box, H, W, halo).any()
    # rows the wrong way round with columns in order: whatever the expression says, tile by tile
    for box in [(3, 40, 20, 19), (3, 40, H - 1, 0), (0, W - 1, 17, 10)]:
        assert lib_rect(box, H, W, halo) == R.rect_of(R.near_map(box, H, W, halo)), box


@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_tile_that_can_see_the_mask_lies_in_the_rectangle(shape, halo):
    H, W = shape
    rng = np.random.default_rng(17 * halo + W)
    xs, ys = corners(W, R.TW, halo), corners(H, R.TH, halo)
    for trial in range(60):
        i, j = sorted(rng.integers(0, len(xs), 2))
        k, l = sorted(rng.integers(0, len(ys), 2))
        x0, x1, y0, y1 = xs[i], xs[j], ys[k], ys[l]
        mask = np.zeros((H, W), bool)
        if trial % 3 == 0:      # the four extreme pixels alone, in random places on the box's sides
            mask[y0, rng.integers(x0, x1 + 1)] = mask[y1, rng.integers(x0, x1 + 1)] = True
            mask[rng.integers(y0, y1 + 1), x0] = mask[rng.integers(y0, y1 + 1), x1] = True
        else:                   # a random fill that touches all four sides
            mask[y0:y1 + 1, x0:x1 + 1] = rng.random((y1 - y0 + 1, x1 - x0 + 1)) < (0.05 if trial % 3 == 1 else 0.6)
            mask[y0, x0] = mask[y1, x1] = True
        box = R.bbox(mask)
        assert box == (x0, x1, y0, y1)
        (tx_lo, tx_hi, ty_lo, ty_hi), n = lib_rect(box, H, W, halo)
        inside = np.zeros_like(R.reach_map(mask, halo))
        inside[ty_lo:ty_hi + 1, tx_lo:tx_hi + 1] = True
        reach = R.reach_map(mask, halo)
        assert not (reach & ~inside).any(), (box, np.argwhere(reach & ~inside))
        assert n == inside.sum() > 0


def test_bad_arguments():
    rect = (C.c_int32 * 4)()
    assert _lib.lib.lg_near_tile_rect(0, 1, 0, 1, 0, 64, 1, rect) == _lib.LG_ERR_INVALID
    assert _lib.lib.lg_near_tile_rect(0, 1, 0, 1, 64, 64, -1, rect) == _lib.LG_ERR_INVALID
    assert _lib.lib.lg_near_tile_rect(0, 1, 0, 1, 64, 64, 1, None) == _lib.LG_ERR_INVALID
