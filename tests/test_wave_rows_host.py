"""The plane kernel's wave-level predicate as the deferred gather evaluates it for one pixel (lg_wave_rows_on_mask: the code
lg_gather_kernel runs), without a device: equal to numpy on random bit rows.  A wave of the plane kernel holds the four rows
(y & ~3) .. (y & ~3) + 3 of a tile over its 64 columns; where none of their pixels lies on the mask it stores +0.0 in every
masked plane, elsewhere a pixel off the mask gets (expression) * 0 -- which can be -0.0 -- so the gather has to know which."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402


def _bit_rows(mask):
    """[H, W] bool -> [H, WW] uint64, bit j of word w = pixel 64 w + j (bits past W are 0)"""
    H, W = mask.shape
    WW = (W + 63) // 64
    padded = np.zeros((H, WW * 64), np.uint64)
    padded[:, :W] = mask
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(H, WW, 64) * weights).sum(axis=2, dtype=np.uint64)


@pytest.mark.parametrize("shape", [(16, 64), (37, 130), (9, 200), (66, 517)])
@pytest.mark.parametrize("density", [0.0, 0.002, 0.05, 1.0])
def test_predicate_equals_numpy(shape, density):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W + int(density * 1e4))
    mask = rng.random((H, W)) < density
    bits = np.ascontiguousarray(_bit_rows(mask))
    WW = bits.shape[1]
    groups = (H + 3) // 4
    padded = np.zeros((groups * 4, WW * 64), bool)
    padded[:H, :W] = mask
    want = padded.reshape(groups, 4, WW, 64).any(axis=(1, 3))   # [group of four rows, word]
    fn = _lib.lib.lg_wave_rows_on_mask
    p = bits.ctypes.data_as(C.c_void_p)
    got = np.array([[fn(p, H, WW, y, w) for w in range(WW)] for y in range(H)])
    np.testing.assert_array_equal(got, want[np.arange(H) // 4].astype(int))


def test_bad_arguments():
    bits = np.zeros((4, 1), np.uint64)
    fn, p = _lib.lib.lg_wave_rows_on_mask, bits.ctypes.data_as(C.c_void_p)
    assert fn(None, 4, 1, 0, 0) == _lib.LG_ERR_INVALID
    assert fn(p, 4, 1, 4, 0) == _lib.LG_ERR_INVALID
    assert fn(p, 4, 1, -1, 0) == _lib.LG_ERR_INVALID
    assert fn(p, 4, 1, 0, 1) == _lib.LG_ERR_INVALID
    assert fn(p, 0, 1, 0, 0) == _lib.LG_ERR_INVALID
