"""What tests/leaf_bb_ref.py predicts for the masks of tests/test_gpu_leaf_edt_fallback.py, asserted on the host: the GPU
test relies on these masks overflowing (or exactly not overflowing) the survivor list of the branch-and-bound pass, and an
edit of a mask that changes that must fail here, without a device."""
import numpy as np
import pytest

from tests import leaf_bb_ref as R


def test_full_list_without_overflow():
    lv = R.bb_survivors(R.lattice(256, 256))
    assert lv[-1] == (1, R.CAP) and max(n for _, n in lv) == R.CAP       # 16 384 at S = 2 and at S = 1: full, not over
    assert not R.bb_overflows(R.lattice(256, 256))


@pytest.mark.parametrize("shape", sorted(R.FALLBACK_SHAPES))
def test_lattices_overflow_at_cells_of_two_pixels(shape):
    H, W = shape
    for name, (m, want) in R.lattice_variants(H, W).items():
        lv = R.bb_survivors(m)
        assert lv[-1] == (2, R.FALLBACK_SHAPES[shape]), (name, lv)
        assert all(n <= R.CAP for _, n in lv[:-1]), (name, lv)
        e = R.exact_field(m >= 1)
        assert np.unravel_index(e.argmax(), e.shape) == want, name
        if name in ("holes", "hole_last_row", "hole_first_and_last_row"):
            assert round(e.max() ** 2) == 5 and (e == e.max()).sum() == 1, name
        if name == "two_holes_tie":
            assert round(e.max() ** 2) == 5 and (e == e.max()).sum() == 2
        if name == "plain":
            assert round(e.max() ** 2) == 2 and (e == e.max()).sum() > 1000


def test_constant_fields_and_sparse_masks_do_not_overflow():
    assert not R.bb_overflows(np.zeros((130, 520), bool))
    assert not R.bb_overflows(np.ones((130, 520), bool))
    frames, _ = R.batch_frames()
    assert [R.bb_overflows(f >= 1) for f in frames] == [False, True, False, False, False]
    assert len(np.unique(frames[0])) > 3 and frames[4].sum() > 0
    for shape in ((40, 4096), (40, 4033)):
        for name, m in R.wide_masks(*shape).items():
            lv = R.bb_survivors(m >= 1)
            assert lv[0][0] == 64 and lv[-1][0] == 1 and max(n for _, n in lv) <= R.CAP, (shape, name, lv)
        w = R.wide_masks(*shape)
        assert not w["first_word_only"][:, 64:].any() and not w["last_word_only"][:, :4032].any()
        assert w["first_and_last_word"][:, :64].any() and w["first_and_last_word"][:, 4032:].any()


def test_wide_dense_noise_prediction():
    """64 x 3840 noise at density 1/2: the best value is a few pixels, every cell of 4 x 4 pixels can still reach it and so can
    half of the cells of 2 x 2: the k_rowedt<4096> route at a width that is no power of two."""
    lv = R.bb_survivors(R.wide_noise() >= 1)
    assert lv[-2] == (4, 15360) and lv[-1][0] == 2 and lv[-1][1] > R.CAP, lv
    assert R.bb_overflows(R.wide_noise() >= 1)
