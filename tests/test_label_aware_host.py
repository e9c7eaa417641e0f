"""Label-aware mode, the arithmetic without a device (include/leafgrasp.h: lg_norm3_host, lg_dilate_words_host,
lg_label_aware_check):

  the norm      min over the zero pixels q of N3(p - q), N3 from lg_norm3_host, equals the oracle's 3x3 chamfer transform bit
                for bit (oracle.distance_transform(img, 3, return_fix=True)) on random 0 / 1 images of 5 x 7 .. 70 x 130, images
                whose zero pixels all lie on the border, and images with one zero pixel.  An image without a zero pixel is not
                in the set: it takes the closed form of the default path.
  the dilation  lg_dilate_words_host (the per-word code of lg_iso_dilate_kernel) equals oracle.dilate for the 30 and 40
                ellipses at widths 64, 65, 100, 130, sources touching every frame edge and corner, random, empty and full images.
  the switch    lg_params keeps its size, label_aware is its last field, and the rule of the entries: 1 needs a label image,
                anything but 0 and 1 is invalid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402

lib = _lib.lib


def norm3(dx, dy):
    dx = np.ascontiguousarray(dx, np.int32).ravel()
    dy = np.ascontiguousarray(dy, np.int32).ravel()
    out = np.empty(dx.size, np.uint32)
    assert lib.lg_norm3_host(dx.ctypes.data, dy.ctypes.data, dx.size, out.ctypes.data) == 0
    return out


def min_over_sources(img):
    """min over the zero pixels q of N3(p - q) for every pixel p, through one table of the norm"""
    H, W = img.shape
    table = norm3(*np.meshgrid(np.arange(W), np.arange(H))).reshape(H, W)   # [dy][dx]
    ys, xs = np.nonzero(img == 0)
    py, px = np.mgrid[:H, :W]
    best = np.full((H, W), 0xFFFFFFFF, np.uint32)
    for y, x in zip(ys, xs):
        best = np.minimum(best, table[np.abs(py - y), np.abs(px - x)])
    return best


def test_norm_values():
    a, b = 62587, 89738   # 0.955, 1.3693 in 16.16
    got = norm3([0, 1, 0, 1, 5, -2, 3], [0, 0, 1, 1, 2, 7, -3])
    assert got.tolist() == [0, a, a, b, 3 * a + 2 * b, 5 * a + 2 * b, 3 * b]
    bad = np.array([20000], np.int32)
    out = np.empty(1, np.uint32)
    assert lib.lg_norm3_host(bad.ctypes.data, bad.ctypes.data, 1, out.ctypes.data) == _lib.LG_ERR_INVALID


def _images():
    rng = np.random.default_rng(33)
    for H, W in [(5, 7), (9, 31), (33, 64), (40, 65), (70, 130)]:
        for density in (0.5, 0.95, 0.995):
            img = (rng.random((H, W)) < density).astype(np.uint8)
            if img.all():
                img[H // 2, W // 3] = 0
            yield f"{H}x{W} random {density}", img
        for name, sl in [("top row", np.s_[0, :]), ("left column", np.s_[:, 0]), ("bottom row", np.s_[H - 1, :]),
                         ("right column", np.s_[:, W - 1])]:
            img = np.ones((H, W), np.uint8)
            line = (rng.random(img[sl].shape) < 0.5).astype(np.uint8)
            line[rng.integers(0, line.size)] = 0
            img[sl] = line
            yield f"{H}x{W} zeros on the {name}", img
        for y, x in [(0, 0), (H - 1, W - 1), (0, W - 1), (H // 2, W // 2)]:
            img = np.ones((H, W), np.uint8)
            img[y, x] = 0
            yield f"{H}x{W} one zero at ({y}, {x})", img


@pytest.mark.parametrize("name,img", list(_images()), ids=[n for n, _ in _images()])
def test_two_passes_equal_the_norm_minimum(name, img):
    assert not img.all()
    _, fix = O.distance_transform(img, 3, return_fix=True)
    got = min_over_sources(img)
    assert np.array_equal(got, fix), (name, np.argwhere(got != fix)[:4])


def pack(mask):
    H, W = mask.shape
    WW = (W + 63) // 64
    padded = np.zeros((H, WW * 64), np.uint8)
    padded[:, :W] = mask
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(H, WW).copy()


def unpack(words, W):
    H = words.shape[0]
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(H, -1), axis=1, bitorder="little")[:, :W]


def host_dilate(mask, k, dirty_tail=False):
    H, W = mask.shape
    bits = pack(mask)
    if dirty_tail and W % 64:   # bits past W must be ignored
        bits[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(W % 64)
    out = np.full_like(bits, 0xA5A5A5A5A5A5A5A5)   # every word must be written
    assert lib.lg_dilate_words_host(bits.ctypes.data, H, W, bits.shape[1], k, out.ctypes.data) == 0
    if W % 64:
        assert not (out[:, -1] >> np.uint64(W % 64)).any(), "bits past W must come out 0"
    return unpack(out, W)


def _sources(H, W, rng):
    edges = {}
    for name, (y, x) in {"top": (0, W // 2), "bottom": (H - 1, W // 3), "left": (H // 2, 0), "right": (H // 3, W - 1),
                         "corner 00": (0, 0), "corner HW": (H - 1, W - 1), "corner 0W": (0, W - 1), "corner H0": (H - 1, 0)}.items():
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        edges[name] = m
    frame = np.zeros((H, W), np.uint8)
    frame[0, :] = frame[-1, :] = 1
    frame[:, 0] = frame[:, -1] = 1
    edges["every edge"] = frame
    edges["2 %"] = (rng.random((H, W)) < 0.02).astype(np.uint8)
    edges["word seams"] = np.zeros((H, W), np.uint8)
    edges["word seams"][H // 2, [c for c in (63, 64, 127, 128) if c < W]] = 1
    edges["empty"] = np.zeros((H, W), np.uint8)
    edges["full"] = np.ones((H, W), np.uint8)
    return edges


@pytest.mark.parametrize("W", [64, 65, 100, 130])
@pytest.mark.parametrize("k", [30, 40])
def test_whole_frame_dilation_equals_the_oracle(W, k):
    rng = np.random.default_rng(W * 100 + k)
    se = O.ellipse_se(k)
    for H in (23, 61):
        for name, m in _sources(H, W, rng).items():
            got = host_dilate(m, k, dirty_tail=True)
            want = O.dilate(m, se)
            assert np.array_equal(got, want), (name, H, W, k, np.argwhere(got != want)[:4])


def test_dilation_other_ellipses_and_bad_arguments():
    rng = np.random.default_rng(5)
    m = (rng.random((37, 150)) < 0.01).astype(np.uint8)
    for k in (1, 2, 3, 31, 63, 64):
        assert np.array_equal(host_dilate(m, k), O.dilate(m, O.ellipse_se(k))), k
    bits = pack(m)
    out = np.empty_like(bits)
    assert lib.lg_dilate_words_host(bits.ctypes.data, 37, 150, 2, 30, out.ctypes.data) == _lib.LG_ERR_INVALID   # WW
    assert lib.lg_dilate_words_host(bits.ctypes.data, 37, 150, 3, 65, out.ctypes.data) == _lib.LG_ERR_INVALID   # k
    assert lib.lg_dilate_words_host(None, 37, 150, 3, 30, out.ctypes.data) == _lib.LG_ERR_INVALID


def test_the_switch():
    assert C.sizeof(_lib.LgParams) == 3 * 8 + 17 * 4 + 9 * 4   # the struct keeps its size
    assert _lib.LgParams._fields_[-1][0] == "label_aware"
    assert _lib.LgParams.label_aware.offset == C.sizeof(_lib.LgParams) - 4
    p = _lib.default_params()
    assert p.label_aware == 0
    assert lib.lg_label_aware_check(C.byref(p), 0) == 0 and lib.lg_label_aware_check(C.byref(p), 1) == 0
    p.label_aware = 1
    assert lib.lg_label_aware_check(C.byref(p), 1) == 0
    assert lib.lg_label_aware_check(C.byref(p), 0) == _lib.LG_ERR_INVALID   # a mask entry has no label image
    for v in (2, -1, 255):
        p.label_aware = v
        assert lib.lg_label_aware_check(C.byref(p), 1) == _lib.LG_ERR_INVALID, v
    assert lib.lg_label_aware_check(None, 1) == _lib.LG_ERR_INVALID
