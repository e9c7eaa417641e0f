"""The stem words by two chains of nested spans (lg_stem_words_host: the code lg_stem_chain_kernel runs), without a device:
equal, word for word, to the oracle's dilate(mask & bottom, ellipse_se(k)) & mask for every k in 1 .. 64, widths of one word, a
full word, a tail of 1 or 2 bits, an even and an odd word count, heights 20 .. 60, a bottom region that starts at row 0, in the
middle and at the last row, masks with set pixels in column 0 and column W - 1, random masks of 2 % and 60 % density, an empty
mask and a full one.  The plan (lg_stem_plan): both chains nested for every k and the library's spans are the oracle's
ellipse; hand-made spans that are not nested take the per-row loop and still equal the oracle."""
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

WIDTHS = [63, 64, 65, 130, 200]
KS = list(range(1, 65))


def pack(mask):
    """[H, W] 0 / 1 -> bit rows [H, WW] uint64, bit j of word w = pixel 64 w + j (bits past W zero)."""
    H, W = mask.shape
    WW = (W + 63) // 64
    padded = np.zeros((H, WW * 64), np.uint8)
    padded[:, :W] = mask
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(H, WW).copy()


def unpack(words, W):
    H = words.shape[0]
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(H, -1), axis=1, bitorder="little")[:, :W]


def oracle_stem(mask, bottom_start, se):
    bottom = np.zeros_like(mask)
    bottom[bottom_start:, :] = 1
    return O.dilate(mask & bottom, se) & mask


def masks_of(H, W, rng):
    border = np.zeros((H, W), np.uint8)
    border[:, 0] = 1
    border[:, W - 1] = 1
    border[rng.integers(0, H, 6), rng.integers(0, W, 6)] = 1
    return {
        "columns 0 and W - 1": border,
        "2 %": (rng.random((H, W)) < 0.02).astype(np.uint8),
        "60 %": (rng.random((H, W)) < 0.60).astype(np.uint8),
        "empty": np.zeros((H, W), np.uint8),
        "full": np.ones((H, W), np.uint8),
    }


def host_words(mask, bottom_start, k):
    H, W = mask.shape
    bits = pack(mask)
    out = np.full_like(bits, 0xA5A5A5A5A5A5A5A5)   # every word must be written
    rc = _lib.lib.lg_stem_words_host(bits.ctypes.data, H, W, bits.shape[1], bottom_start, k, out.ctypes.data)
    assert rc == 1, rc   # the chains ran
    return out


@pytest.mark.parametrize("W", WIDTHS)
def test_every_ellipse_equals_the_oracle(W):
    rng = np.random.default_rng(1000 + W)
    nonzero = 0
    for k in KS:
        H = 20 + (7 * k + W) % 41                     # 20 .. 60
        se = O.ellipse_se(k)
        ms = masks_of(H, W, rng)
        for bottom_start in (0, H // 2, H - 1):
            for name, m in ms.items():
                want = oracle_stem(m, bottom_start, se)
                got = host_words(m, bottom_start, k)
                assert np.array_equal(got, pack(want)), (k, H, W, bottom_start, name,
                                                         np.argwhere(unpack(got, W) != want)[:5])
                nonzero += int(want.sum() > 0)
    assert nonzero >= 3 * 3 * len(KS)   # nothing here compares zeros with zeros only


def test_heights_at_both_ends():
    rng = np.random.default_rng(5)
    for H in (20, 60):
        for k in (1, 2, 29, 30, 31, 63, 64):
            m = (rng.random((H, 130)) < 0.3).astype(np.uint8)
            for bs in (0, H // 2, H - 1):
                assert np.array_equal(host_words(m, bs, k), pack(oracle_stem(m, bs, O.ellipse_se(k))))


def plan_of(k=0, spans=None, anchor=0):
    i0 = C.c_int32(-1)
    arr = [(C.c_int8 * 64)() for _ in range(4)]
    if spans is None:
        rc = _lib.lib.lg_stem_plan(k, 0, 0, None, None, C.byref(i0), *arr)
    else:
        lo = (C.c_int8 * len(spans))(*[s[0] for s in spans])
        hi = (C.c_int8 * len(spans))(*[s[1] for s in spans])
        rc = _lib.lib.lg_stem_plan(0, len(spans), anchor, lo, hi, C.byref(i0), *arr)
    return rc, i0.value, [list(a) for a in arr]


@pytest.mark.parametrize("k", KS)
def test_plan_of_every_ellipse_is_two_nested_chains(k):
    rc, i0, (lo, hi, dlo, dhi) = plan_of(k)
    assert rc == 1
    se = O.ellipse_se(k)
    a = k // 2
    for i in range(k):   # the library's spans are the oracle's ellipse, one contiguous span per row
        cols = np.nonzero(se[i])[0]
        assert cols.size and cols[-1] - cols[0] + 1 == cols.size
        assert (lo[i], hi[i]) == (cols[0] - a, cols[-1] - a)
    width = [hi[i] - lo[i] for i in range(k)]
    assert width[i0] == max(width)
    for i in range(k):
        if i == i0:
            continue
        prev = i + 1 if i < i0 else i - 1
        assert lo[prev] <= lo[i] and hi[i] <= hi[prev]            # nested towards the widest row
        assert (dlo[i], dhi[i]) == (lo[prev] - lo[i], hi[prev] - hi[i])
        assert dlo[i] <= 0 <= dhi[i]
    assert lo[0] <= 0 <= hi[0] and lo[k - 1] <= 0 <= hi[k - 1]
    assert min(lo[:k]) >= -32 and max(hi[:k]) <= 32               # the 192-bit segment is enough
    if k == 30:   # the work the chains save: 17 dilations that do anything for 30 rows
        steps = sum(1 for i in range(k) if i != i0 and (dlo[i], dhi[i]) != (0, 0))
        assert steps <= 17, steps


def se_matrix(spans, anchor):
    n = len(spans)
    se = np.zeros((n, n), np.uint8)
    for i, (lo, hi) in enumerate(spans):
        if lo <= hi:
            se[i, anchor + lo:anchor + hi + 1] = 1
    return se


def spans_words(mask, bottom_start, spans, anchor, algo):
    H, W = mask.shape
    bits = pack(mask)
    out = np.full_like(bits, 0x5A5A5A5A5A5A5A5A)
    lo = (C.c_int8 * len(spans))(*[s[0] for s in spans])
    hi = (C.c_int8 * len(spans))(*[s[1] for s in spans])
    rc = _lib.lib.lg_stem_words_host_spans(bits.ctypes.data, H, W, bits.shape[1], bottom_start, len(spans), anchor, lo, hi, algo,
                                           out.ctypes.data)
    return rc, out


# (the oracle's dilate anchors an n x n element at n // 2, rows and columns)
NOT_NESTED = [
    ([(-3, -1), (0, 2), (-1, 1), (-3, 3), (1, 3), (-2, 0), (0, 0)], 3),       # rows that stick out of their inner neighbours
    ([(-1, 1), (-2, 2), (1, 0), (-2, 2), (-1, 1)], 2),                         # an empty row
    ([(1, 2), (-2, 2), (-2, 2), (-1, 1), (0, 0)], 2),                          # an end row that does not hold column 0
]
NESTED = [
    ([(0, 0), (-1, 0), (-1, 2), (-3, 3), (-3, 3), (-2, 3), (0, 1)], 3),       # lopsided but nested
    ([(0, 0)], 0),
    ([(-1, 0), (0, 0)], 1),                                                     # the widest row is an end row
]


@pytest.mark.parametrize("case", range(len(NOT_NESTED) + len(NESTED)))
def test_hand_made_spans(case):
    nested = case >= len(NOT_NESTED)
    spans, anchor = (NESTED[case - len(NOT_NESTED)] if nested else NOT_NESTED[case])
    assert plan_of(spans=spans, anchor=anchor)[0] == (1 if nested else 0)
    se = se_matrix(spans, anchor)
    rng = np.random.default_rng(40 + case)
    checked = 0
    for H, W in ((24, 63), (33, 130), (41, 200)):
        for name, m in masks_of(H, W, rng).items():
            for bs in (0, H // 2, H - 1):
                want = pack(oracle_stem(m, bs, se))
                rc, got = spans_words(m, bs, spans, anchor, 1)
                assert rc == (1 if nested else 0)          # spans that are not nested take the per-row loop
                assert np.array_equal(got, want), (spans, H, W, bs, name)
                rc, got = spans_words(m, bs, spans, anchor, 0)
                assert rc == 0 and np.array_equal(got, want), (spans, H, W, bs, name)
                checked += int(want.any())
    assert checked > 10


def test_bad_arguments():
    bits = np.zeros((8, 1), np.uint64)
    out = np.zeros_like(bits)
    f = _lib.lib.lg_stem_words_host
    assert f(bits.ctypes.data, 8, 64, 1, 0, 0, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert f(bits.ctypes.data, 8, 64, 1, 0, 65, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert f(bits.ctypes.data, 8, 64, 2, 0, 5, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert f(None, 8, 64, 1, 0, 5, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert f(bits.ctypes.data, 8, 64, 1, 9, 5, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert _lib.lib.lg_stem_plan(65, 0, 0, None, None, None, None, None, None, None) == _lib.LG_ERR_INVALID
