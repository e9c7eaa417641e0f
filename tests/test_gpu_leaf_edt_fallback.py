"""The clutter arg-max of the leaf stage on its two routes, told apart by lg_debug_leaf_fallback: the branch-and-bound pass
on the bit mask (lg_leaf.hip::k_edt_bb) and, when a survivor list overflows, the full transform for the whole batch
(k_coldist, k_rowedt<512 | 1024 | 2048 | 4096>, k_rowbest).  Masks that must overflow and masks that must not come from
tests/leaf_bb_ref.py, whose predictions tests/test_leaf_bb_ref.py asserts without a device; here the device's flag must equal
the prediction and both extrema must be np.argmax / np.argmin of scipy's exact field.  Also the stage's width edges: the
64th word of a bit row (W = 4096, 4033) and the refusal of W = 4097."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import leaf_bb_ref as R  # noqa: E402

_P = np.array([[500.0, 0, 240, -20], [0, 500, 180, 0], [0, 0, 1, 0]])


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


@pytest.fixture
def ols(L):
    s = L.OptimalLeafSelector("cuda:0")
    s.set_camera_params(_P)
    return s


def _extrema(lab):
    e = R.exact_field(lab >= 1)
    return (tuple(int(v) for v in np.unravel_index(e.argmin(), e.shape)),
            tuple(int(v) for v in np.unravel_index(e.argmax(), e.shape)))


def _stats(ols, lab, depth=None):
    d = np.full(lab.shape, 0.5, np.float32) if depth is None else depth
    return ols.leaf_statistics(torch.from_numpy(lab).cuda(), torch.from_numpy(d).cuda())


def _check(ols, lab, want_flag, what):
    rows, (mn, mx), _ = _stats(ols, lab)
    flags = ols.edt_fallback_frames()
    emn, emx = _extrema(lab)
    print(what, lab.shape, "flag", flags, "predicted", want_flag, "arg-max", mx, "exact", emx)
    assert flags == [want_flag], what
    assert mx == emx and mn == emn, what
    return rows


def test_full_list_is_not_an_overflow(ols):
    """Exactly LGL_QCAP / 4 survivors at cells of two pixels and of one: the last entry that fits."""
    lab = R.lattice(256, 256)
    assert R.bb_survivors(lab)[-1] == (1, R.CAP)
    assert ols.edt_fallback_frames() == []                                   # no call yet
    _check(ols, lab, False, "full list")


@pytest.mark.parametrize("shape", sorted(R.FALLBACK_SHAPES))
def test_fallback_at_every_row_kernel_width(ols, shape):
    """258 x 256 -> k_rowedt<512>, 130 x 520 -> <1024>, 66 x 1030 -> <2048>, 34 x 2050 and 18 x 4096 -> <4096>."""
    for name, (lab, want) in R.lattice_variants(*shape).items():
        assert R.bb_overflows(lab), name
        _check(ols, lab, True, name)
        assert _extrema(lab)[1] == want, name
    # and back on the branch-and-bound route on the same handle
    speck = np.zeros(shape, np.int16)
    speck[shape[0] // 2, shape[1] // 3] = 1
    _check(ols, speck, False, "speck")


def test_one_overflowing_frame_in_a_batch(ols):
    """The fallback runs for the whole batch: every frame's arg-max is rewritten by it, every frame's statistics stay."""
    frames, depth = R.batch_frames()                                         # 130 x 520
    want_flags = [R.bb_overflows(f >= 1) for f in frames]
    assert want_flags == [False, True, False, False, False]
    lab = torch.from_numpy(np.stack(frames)).cuda()
    dep = torch.from_numpy(np.stack([depth] * len(frames))).cuda()
    out = ols.leaf_statistics_batch(lab, dep)
    assert ols.edt_fallback_frames() == want_flags
    singles = []
    for b, f in enumerate(frames):
        single = ols.leaf_statistics(lab[b], dep[b])
        assert ols.edt_fallback_frames() == [want_flags[b]], b
        singles.append(single)
        assert out[b][1] == single[1] == _extrema(f), b
        assert len(out[b][0]) == len(single[0])
        for x, y in zip(out[b][0], single[0]):
            assert all(x[k] == y[k] for k in ("id", "area", "touches_border", "sum_x", "sum_y", "median_depth")), (b, x["id"])
            # f64 atomics: the accumulation order differs with the grid -> last-bit differences
            assert abs(x["sum_depth"] - y["sum_depth"]) <= 1e-9 * abs(y["sum_depth"]) + 1e-12
            assert abs(x["sum_ray"] - y["sum_ray"]) <= 1e-9 * abs(y["sum_ray"]) + 1e-12
    assert out[2][1] == ((0, 0), (0, 0)) and out[3][1] == ((0, 0), (0, 0))
    # the selection entry runs the same stage: it reports through the same export
    ols.select_optimal_leaves_batch(lab, dep)
    assert ols.edt_fallback_frames() == want_flags
    again = ols.leaf_statistics_batch(lab[:1], dep[:1])
    assert ols.edt_fallback_frames() == [False]
    assert again[0][1] == singles[0][1] == _extrema(frames[0])


@pytest.mark.parametrize("shape", [(40, 4096), (40, 4033)])
def test_widest_frames_on_the_branch_and_bound_route(ols, shape):
    """Bit rows of 64 words: word 63 has nothing to its right (k_rowocc's lane < WW, edt_point_wave_occ's w0 < 63)."""
    H, W = shape
    rng = np.random.default_rng(29)
    depth = rng.uniform(0.3, 0.9, shape).astype(np.float32)
    for name, lab in R.wide_masks(H, W).items():
        assert not R.bb_overflows(lab), name
        rows, (mn, mx), _ = _stats(ols, lab, depth)
        assert ols.edt_fallback_frames() == [False], name
        assert (mn, mx) == _extrema(lab), name
        lm = lab == 1
        assert len(rows) == 1 and rows[0]["id"] == 1 and rows[0]["area"] == int(lm.sum()), name
        assert rows[0]["sum_x"] == float(np.where(lm)[1].sum()) and rows[0]["median_depth"] == np.median(depth[lm]), name


def test_wide_dense_noise(ols):
    lab = R.wide_noise()
    _check(ols, lab, R.bb_overflows(lab), "64 x 3840 noise")


def test_width_above_4096_is_refused(L, ols):
    lab = np.zeros((8, 4097), np.int16)
    lab[3, 4000:4096] = 2
    dep = np.full(lab.shape, 0.5, np.float32)
    with pytest.raises(L.LgError):
        _stats(ols, lab, dep)
    assert ols.edt_fallback_frames() == []
    assert ols.select_optimal_leaf(torch.from_numpy(lab).cuda(), torch.from_numpy(dep).cuda()) is None
    ok = lab[:, :4096].copy()                                                # the handle still works
    rows, (mn, mx), _ = _stats(ols, ok)
    assert (mn, mx) == _extrema(ok) and rows[0]["area"] == 96
