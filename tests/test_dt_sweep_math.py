"""What form 6 of the sweep-free distance transform (lg_dtsweep_kernel, csrc/lg_dt.hip) does beyond identity (1) of
tests/test_dt_band_math.py, restated in NumPy and checked against the integers of the oracle's two-pass chamfer transform:
  * U and D run over the rows of the mask's bounding box only, and over a span of `lanes` x E columns that starts at the box's
    first column rounded down to a multiple of 4 (E = the smallest of 4, 8, 16, 32 that holds the box); cells above / below the
    box and beside the span count 0 inside the image and "no path" outside it, run distances are read only where
    lg_hrun_kernel wrote them (the 64-column words of the box) and count 0 elsewhere in the image;
  * U is parked on the upper half of the rows and D on the lower half; past mid-height each run takes the minimum with the row
    the other parked.  A run never reads a row that was not parked before the hand-over.
The device has 64 lanes; the emulation takes fewer so that small images reach every E and spans that end on the box's edge."""
import numpy as np
import pytest

from tests.test_dt_band_math import A, B, C, CAP, INF, _big_cases, _ref, _runs
from tests.test_dt_search_math import _cases


def _step(p1, f1, p2, f2, ah):
    """One row of the recurrence over the span.  p1 / p2 = the rows one / two steps back; f = (the cells left of the span, the
    two cells right of it) of that row: a row keeps what it was set with when it becomes the row two steps back."""
    n = p1.size
    q1 = np.concatenate(([f1[0], f1[0]], p1, [f1[1], f1[2]]))
    q2 = np.concatenate(([f2[0]], p2, [f2[1]]))
    mc = np.minimum(np.minimum(q1[0:n], q1[4:4 + n]), np.minimum(q2[0:n], q2[2:2 + n])) + C
    mb = np.minimum(q1[1:1 + n], q1[3:3 + n]) + B
    return np.minimum(np.minimum(ah, p1 + A), np.minimum(mb, mc))


def _sweep(mask, lanes):
    """-> (d of the whole image as form 6 computes it, E)"""
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    by0, by1, bx0, bx1 = ys.min(), ys.max(), xs.min(), xs.max()
    sx0 = bx0 & ~3
    E = next(e for e in (4, 8, 16, 32) if lanes * e >= bx1 - sx0 + 1)
    xe = sx0 + lanes * E
    cols = np.arange(sx0, xe)
    col_in = cols < W
    hx0, hx1 = (bx0 >> 6) << 6, min(W, ((bx1 >> 6) + 1) << 6)
    written = (cols >= hx0) & (cols < hx1)
    h = _runs(mask)
    fl = 0 if sx0 > 0 else INF
    fr0, fr1 = (0 if xe < W else INF), (0 if xe + 1 < W else INF)

    def ah_row(y):
        return np.where(written, A * h[y, np.minimum(cols, W - 1)], np.where(col_in, 0, A * CAP))

    def edge(y):   # a row beside the box and its fills
        if 0 <= y < H:
            return np.where(col_in, 0, INF), (fl, fr0, fr1)
        return np.full(cols.size, INF, np.int64), (INF, INF, INF)

    n = by1 - by0 + 1
    na = n // 2
    parked = np.full((H, cols.size), -1, np.int64)
    final = np.full((H, cols.size), -1, np.int64)
    runs = []
    for y0, d, cnt_a in ((by0, 1, na), (by1, -1, n - na)):
        (p2, f2), (p1, f1) = edge(y0 - 2 * d), edge(y0 - d)
        runs.append({"p1": p1, "p2": p2, "f1": f1, "f2": f2, "y": y0, "d": d, "cnt_a": cnt_a})

    def advance(s):
        v = _step(s["p1"], s["f1"], s["p2"], s["f2"], ah_row(s["y"]))
        s["p2"], s["f2"] = s["p1"], s["f1"]
        s["p1"], s["f1"] = v, (fl, fr0, fr1)
        s["y"] += s["d"]
        return s["y"] - s["d"], v

    for s in runs:                       # up to mid-height: park
        for _ in range(s["cnt_a"]):
            y, v = advance(s)
            assert parked[y, 0] == -1
            parked[y] = v
    for s in runs:                       # (the barrier)  past mid-height: combine with what the other parked
        for _ in range(n - s["cnt_a"]):
            y, v = advance(s)
            assert (parked[y] >= 0).all() and final[y, 0] == -1, "a row is requested that the other run did not park"
            final[y] = np.minimum(v, parked[y])
    assert (final[by0:by1 + 1] >= 0).all()
    out = np.zeros((H, W), np.int64)
    keep = cols[col_in]
    out[by0:by1 + 1, keep[0]:keep[-1] + 1] = final[by0:by1 + 1][:, col_in]
    return out, E


def test_step_with_no_path_fills_is_the_band_step():
    from tests.test_dt_band_math import _step as band_step
    rng = np.random.default_rng(0)
    for _ in range(20):
        p1, p2, ah = (rng.integers(0, 1 << 24, 37) for _ in range(3))
        np.testing.assert_array_equal(_step(p1, (INF,) * 3, p2, (INF,) * 3, ah), band_step(p1, p2, ah))


@pytest.mark.parametrize("lanes", [2, 3, 16])
def test_sweep_over_box_and_span_with_the_hand_over_at_mid_height(lanes):
    seen, bad = set(), 0
    for mask in _cases(240, 5) + _cases(60, 11):
        xs = np.nonzero(mask)[1]
        if xs.max() - (xs.min() & ~3) + 1 > 32 * lanes:
            continue
        got, E = _sweep(mask, lanes)
        seen.add(E)
        bad += int((got != _ref(mask)).sum())
    assert bad == 0
    assert seen == ({4, 8, 16, 32} if lanes < 16 else {4, 8})


def test_sweep_on_the_band_generators():
    seen, bad = set(), 0
    for mask in _big_cases(24, 13):
        got, E = _sweep(mask, 11)
        seen.add(E)
        bad += int((got != _ref(mask)).sum())
    assert bad == 0 and seen >= {16, 32}


def _box(H, W, y0, y1, x0, x1, holes=False):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1 + 1, x0:x1 + 1] = 1
    if holes:
        m[(y0 + y1) // 2, (x0 + x1) // 2] = 0
    return m


def test_boxes_at_the_corners_and_spans_that_end_on_the_box():
    H, W, lanes = 23, 50, 3
    cases = []
    for rows in (1, 2, 3, 4, 7, H):                      # the hand-over row: 1, 2, 3, even, odd, the whole height
        for y0 in {0, H - rows, (H - rows) // 2}:
            for x0, x1 in ((0, 11), (0, 12), (W - 12, W - 1), (W - 13, W - 1), (0, W - 2), (1, W - 1), (17, 17), (0, 0), (W - 1, W - 1)):
                cases.append(_box(H, W, y0, y0 + rows - 1, x0, x1))
    for E in (4, 8, 16):                                 # lane boundaries on the box's first and last column, and one past them
        for x0 in (0, 4, 5, 6, 7, 8):
            for wd in (lanes * E - 1, lanes * E, lanes * E + 1):
                if x0 + wd <= W:
                    cases.append(_box(H, W, 3, 15, x0, x0 + wd - 1, holes=True))
    assert len(cases) > 150
    bad = 0
    for m in cases:
        if m.all():
            m[H // 2, W // 2] = 0                        # (the search needs a zero pixel in the image)
        bad += int((_sweep(m, lanes)[0] != _ref(m)).sum())
    assert bad == 0
