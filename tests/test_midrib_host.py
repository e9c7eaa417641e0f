"""detect_midrib without a device: the CLAHE restatement against hand-worked values, tile geometry, and the library's host
ridge walk (lg_midrib_walk, the arithmetic the device walk runs) against the NumPy restatement of the reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import leafgrasp_amd as L  # noqa: E402
from leafgrasp_amd import _lib  # noqa: E402

from tests import midrib_ref as R  # noqa: E402


def test_selector_mirrors_detect_midrib():
    assert hasattr(L.GraspPointSelector, "detect_midrib")
    assert hasattr(L.GraspPointSelector, "detect_midrib_batch")
    assert callable(L.clahe)


@pytest.mark.parametrize("H,W,tile", [(1080, 1920, (240, 135)), (1080, 1442, (181, 136)), (517, 733, (92, 65)),
                                      (1080, 1440, (180, 135)), (5, 7, (1, 1))])
def test_clahe_tile_size(H, W, tile):
    # 1080 x 1442: 1442 % 8 != 0 pads BOTH dimensions, so the divisible 1080 rows gain 8 more (1088 / 8 = 136)
    assert R.clahe_tile_size(H, W, 8, 8) == tile


def test_clahe_hand_worked_lut():
    # 16 x 16, 2 x 2 tiles of 8 x 8 = 64 pixels, every tile: 40 pixels of 10 (rows 0-4) and 24 of 200 (rows 5-7).
    # clipLimit 40: clip = int(40 * 64 / 256) = 10.  bin 10: 40 -> 10 (30 clipped), bin 200: 24 -> 10 (14 clipped);
    # 44 clipped: batch 0, residual 44, step 256 // 44 = 5 -> +1 at bins 0, 5, ..., 215.
    # lut[i] = rint(cumsum[i] * 255 / 64), 255 / 64 = 3.984375:
    tile = np.full((8, 8), 10, np.uint8)
    tile[5:] = 200
    img = np.tile(tile, (2, 2))
    expected = {0: 4,      # cumsum 1   -> 3.984
                4: 4,      #        1
                5: 8,      #        2   -> 7.969
                9: 8,      #        2
                10: 52,    #  3 + 10 = 13 -> 51.797
                199: 199,  # 40 + 10 = 50 -> 199.22
                200: 243,  # 41 + 20 = 61 -> 243.05
                214: 251,  # 43 + 20 = 63 -> 251.02
                215: 255, 255: 255}   # 64
    luts = R.clahe_luts(img, 40.0, (2, 2))
    for t in luts.reshape(4, 256):
        for i, v in expected.items():
            assert t[i] == v, (i, t[i], v)
    out = R.clahe(img, 40.0, (2, 2))
    assert (out[img == 10] == 52).all() and (out[img == 200] == 243).all()


def test_clahe_lut_rounds_half_to_even():
    # 10 x 2, tiles (1, 2): tiles of 10 x 1, lut scale 255 / 10 = 25.5 exactly.  Row 0 = three 0s, two 1s, four 2s, one 3:
    # cumsum 3 -> 76.5 -> 76 (half up would give 77), 5 -> 127.5 -> 128, 9 -> 229.5 -> 230, 10 -> 255
    img = np.array([[0, 0, 0, 1, 1, 2, 2, 2, 2, 3], [5] * 10], np.uint8)
    lut = R.clahe_luts(img, 0.0, (1, 2))[0, 0]
    assert (lut[0], lut[1], lut[2], lut[3]) == (76, 128, 230, 255)
    out = R.clahe(img, 0.0, (1, 2))
    assert out[0].tolist() == [76, 76, 76, 128, 128, 230, 230, 230, 230, 255]


def _walk_lib(enh, mask, orient):
    H, W = mask.shape
    out, st = (C.c_int32 * 4)(), C.c_int32(-9)
    found = orient[0] is not None
    o = (C.c_float * 5)(*([orient[0], orient[1], orient[2], orient[3][0], orient[3][1]] if found else [0.0] * 5))
    e = np.ascontiguousarray(enh, np.uint8)
    m = np.ascontiguousarray(mask, np.uint8)
    rc = _lib.lib.lg_midrib_walk(e.ctypes.data, m.ctypes.data, H, W, int(found), o, out, C.byref(st))
    assert rc == 0
    if st.value == 0:
        return 0, ((out[0], out[1]), (out[2], out[3]))
    assert list(out) == [-1] * 4
    return st.value, None


def _f32(v):
    return float(np.float32(v))


def _random_case(rng):
    H, W = int(rng.integers(6, 90)), int(rng.integers(6, 90))
    kind = rng.integers(0, 4)
    if kind == 0:
        mask = (rng.random((H, W)) < rng.uniform(0.3, 1.0)).astype(np.uint8)
    elif kind == 1:
        mask = np.ones((H, W), np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        mask = (((xx - rng.uniform(0, W)) / rng.uniform(3, W)) ** 2 + ((yy - rng.uniform(0, H)) / rng.uniform(3, H)) ** 2 <= 1)
        mask = mask.astype(np.uint8) * np.uint8(rng.integers(1, 256))
    levels = int(rng.choice([2, 3, 8, 256]))   # few levels: ties in the maximum
    enh = rng.integers(0, levels, (H, W)).astype(np.uint8)
    if rng.random() < 0.08:
        return enh, mask, (None, None, None, None)
    r = rng.random()
    if r < 0.15:
        angle = float(rng.choice([np.float32(np.pi), np.float32(np.pi / 2), np.float32(np.pi / 4), np.float32(3 * np.pi / 4)]))
    else:
        angle = _f32(rng.uniform(1e-6, np.pi))
    major = _f32(rng.uniform(0.0, 2.2 * max(H, W)))
    m = rng.random()
    if m < 0.15:
        minor = _f32(rng.uniform(0.0, 6.0))            # cv2.line's thickness 0
    elif m < 0.35:
        minor = _f32(rng.uniform(6.0, 12.0))           # ww == 1: linspace(-1, 1, 1) == [-1]
    else:
        minor = _f32(rng.uniform(6.0, max(12.0, major)))
    major = max(major, minor)
    cx = _f32(rng.uniform(-0.3 * W, 1.3 * W))           # centre-line points leave the frame
    cy = _f32(rng.uniform(-0.3 * H, 1.3 * H))
    return enh, mask, (angle, major, minor, (cx, cy))


def test_walk_matches_reference_restatement():
    rng = np.random.default_rng(1234)
    seen = set()
    for i in range(600):
        enh, mask, orient = _random_case(rng)
        exp = R.midrib_walk(enh, mask, orient)
        got = _walk_lib(enh, mask, orient)
        assert got == exp, (i, orient, mask.shape, got, exp)
        seen.add(exp[0])
    assert seen == {0, 1, 2, 3}, seen


def test_walk_truncates_toward_zero():
    # angle with cos 0.6, sin 0.8, major 10.2: dx = int(5.1 * 0.6) = 3, dy = int(5.1 * 0.8) = 4; minor 6.5: ww = 1, s = -1,
    # perp = (-0.8, 0.6).  Centre (10, 4): step t = 0 is (7, 0), its sample (7.8, -0.6) lands on (7, 0) -- int() truncates
    # toward zero, floor would put it at y = -1, off the frame.  t = 1: centre (13, 8), sample (13.8, 7.4) -> (13, 7).
    enh = np.zeros((20, 20), np.uint8)
    mask = np.ones((20, 20), np.uint8)
    orient = (_f32(np.arctan2(0.8, 0.6)), 10.2, 6.5, (10.0, 4.0))
    assert R.midrib_walk(enh, mask, orient) == (0, ((7, 0), (13, 7)))
    assert _walk_lib(enh, mask, orient) == (0, ((7, 0), (13, 7)))


def test_walk_first_maximum_wins():
    # horizontal axis: angle float32(pi), major 40 -> dx = int(20 * cos) = -19 (cos is just above -1), dy = 0; minor 30 ->
    # ww = 5 samples along the column, perp = (0, -5): s = -1, -0.5, 0, 0.5, 1 sample rows y + 5, y + 2.5, y, y - 2.5, y - 5.
    # Rows 15-24 hold the maximum 9: at y = 20 rows 22, 20, 17 and 15 tie, and the first sample (row 22) wins (np.argmax)
    enh = np.zeros((40, 40), np.uint8)
    enh[15:25, :] = 9
    mask = np.ones((40, 40), np.uint8)
    orient = (float(np.float32(np.pi)), 40.0, 30.0, (20.0, 20.0))
    exp = R.midrib_walk(enh, mask, orient)
    assert exp[0] == 0
    assert _walk_lib(enh, mask, orient) == exp
    assert exp[1][0][1] == 22, exp


def test_walk_rejects_bad_arguments():
    out, st = (C.c_int32 * 4)(), C.c_int32()
    z = np.zeros((4, 4), np.uint8)
    assert _lib.lib.lg_midrib_walk(None, z.ctypes.data, 4, 4, 0, None, out, C.byref(st)) == _lib.LG_ERR_INVALID
    assert _lib.lib.lg_midrib_walk(z.ctypes.data, z.ctypes.data, 4, 4, 1, None, out, C.byref(st)) == _lib.LG_ERR_INVALID
