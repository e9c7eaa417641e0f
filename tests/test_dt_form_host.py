"""Which form of the sweep-free row search a batch takes (lg_dt_form_host: the table lg_select_grasp* and lg_score_maps use,
csrc/lg_dt.h), without a device.  Forms: 1 = every row searched, 5 = seed row pairs + stencil bands (needs sixteen rows and
columns), 6 = one register sweep per frame (the same, and at most 2048 columns); `forced` is LG_DT_SEARCH_ALGO, 0 = by size.
The table is restated here in words of its own and compared at its edges."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402

SMALL = 64 * 1080 * 1920   # pixels in a batch up to which one launch of form 1 wins


def form(forced, n, H, W):
    return int(_lib.lib.lg_dt_form_host(forced, n, H, W))


def expected(forced, n, H, W):
    roomy = H >= 16 and W >= 16
    sweep = roomy and W <= 2048
    if forced == 1:
        return 1
    if forced == 5:
        return 5 if roomy else 1
    if forced == 0 and n * H * W <= SMALL:
        return 1
    return 6 if sweep else 5 if roomy else 1


@pytest.mark.parametrize("forced", [0, 1, 5, 6])
def test_the_table_at_its_edges(forced):
    for H in (12, 15, 16, 17, 1080, 2160):
        for W in (15, 16, 17, 40, 1920, 2048, 2052, 3840, 4096):
            at = SMALL // (H * W)   # the largest batch that is still small
            for n in (1, 2, at, at + 1, 4000):
                if n >= 1:
                    assert form(forced, n, H, W) == expected(forced, n, H, W), (forced, n, H, W)


def test_the_batch_size_threshold_is_inclusive():
    assert form(0, 64, 1080, 1920) == 1      # n H W == 64 * 1080 * 1920
    assert form(0, 65, 1080, 1920) == 6      # one frame more
    assert form(0, 16, 2160, 3840) == 1      # the same number of pixels at 4K
    assert form(0, 17, 2160, 3840) == 5


def test_the_register_sweep_ends_at_2048_columns():
    assert form(0, 4000, 24, 2048) == 6 and form(6, 1, 24, 2048) == 6
    assert form(0, 4000, 24, 2052) == 5 and form(6, 1, 24, 2052) == 5
    assert form(5, 1, 24, 2048) == 5 and form(5, 4000, 24, 2048) == 5   # forced stays forced


@pytest.mark.parametrize("forced", [0, 5, 6])
def test_sixteen_rows_and_columns(forced):
    n = 1 << 20   # past the small-batch threshold at every size below
    assert form(forced, n, 15, 520) == 1 and form(forced, n, 520, 15) == 1
    want = 5 if forced == 5 else 6
    assert form(forced, n, 16, 520) == want and form(forced, n, 520, 16) == want and form(forced, n, 16, 16) == want


def test_forced_one_level_everywhere():
    assert form(1, 4000, 1080, 1920) == 1 and form(1, 4000, 2160, 3840) == 1 and form(1, 1, 12, 40) == 1


def test_the_corner_that_once_took_the_two_level_search():
    assert 4000 * 12 * 4096 > SMALL
    assert form(0, 4000, 12, 4096) == 1
