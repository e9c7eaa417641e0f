"""Form 6 of the sweep-free distance transform (LG_DT_SEARCH_ALGO=6, lg_dtsweep_kernel): one workgroup per frame, wave 0 runs
the 5 x 5 chamfer stencil downwards over the bounding box's rows, wave 1 upwards, lane = E columns of a span of 64 E columns
(E = 4, 8, 16, 32 by the box's width), hand-over at mid-height (the arithmetic: tests/test_dt_sweep_math.py).  distance_map,
max d_in and max d_out must be the oracle's two-pass transform bit for bit.  The shapes are the smallest that reach every
path: every E at one width, widths that are no multiple of 4 (scalar loads and stores), a span that ends past the image, a
width beyond 2048 columns (the form falls back to 5)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests.test_gpu_dt_bands import _hard_masks, _window_case  # noqa: E402

SHAPES = [(96, 128), (131, 258), (150, 333), (40, 520), (24, 1030), (24, 2048), (24, 2052)]
SCALE = np.float32(1.0 / 65536.0)


def _selector(algo):
    import leafgrasp_amd as L

    assert torch.cuda.is_available()
    env = {"LG_DT_SEARCH": "1", "LG_DT_SEARCH_ALGO": algo}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:   # the options are read when a handle is created
        s = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
        s.set_camera_params(O.synthetic_scene(64, 64, 0)[2])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return s


@pytest.fixture(scope="module")
def sel():
    return _selector("6")


def _shape_masks(H, W):
    """name -> mask: what every shape has to pass."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = {}

    def rect(y0, y1, x0, x1):   # inclusive
        m = np.zeros((H, W), np.uint8)
        m[y0:y1 + 1, x0:x1 + 1] = 1
        return m
    # a span of every E class this width has room for: 64 E >= the box's width (from its first column rounded down to 4)
    for wd in (200, 252, 257, 400, 900, 1100, 2000):
        for x0 in (4, 5, W - wd):
            if 0 <= x0 and x0 + wd <= W:
                m = rect(2, H - 3, x0, x0 + wd - 1) & (((xx + 2 * yy) % 9 != 0) | (yy % 4 != 1)).astype(np.uint8)
                m[2, x0] = m[H - 3, x0 + wd - 1] = 1
                out[f"span: box of {wd} columns from {x0}"] = m
    for rows in (1, 2, 3, 6, 7):   # the hand-over row
        out[f"box of {rows} rows"] = rect(H // 3, H // 3 + rows - 1, W // 5, W - W // 4)
        out[f"box of {rows} rows at the top"] = rect(0, rows - 1, 3, W // 2)
        out[f"box of {rows} rows at the bottom"] = rect(H - rows, H - 1, W // 3, W - 1)
    out["leaf on the top border"] = rect(0, H // 3, W // 4, W // 2 + 9)
    out["leaf on the bottom border"] = rect(H - H // 3, H - 1, W // 3, W - 7)
    out["leaf on the left border"] = rect(H // 4, H // 2 + 5, 0, W // 3)
    out["leaf on the right border"] = rect(H // 3, H - 4, W - W // 3, W - 1)
    out["leaf in the first corner"] = rect(0, 5, 0, 9)
    out["leaf in the top right corner"] = rect(0, 6, W - 11, W - 1)
    out["leaf in the bottom left corner"] = rect(H - 5, H - 1, 0, 6)
    out["leaf in the last corner"] = rect(H - 7, H - 1, W - 9, W - 1)
    out["full-width band"] = rect(H // 5, (4 * H) // 5, 0, W - 1)
    r = np.hypot(yy - H / 2, xx - W / 2)
    out["ring"] = ((r < 0.45 * H) & (r > 0.2 * H)).astype(np.uint8)
    m = rect(H // 4, (3 * H) // 4, W // 4, (3 * W) // 4); m[H // 3:(2 * H) // 3, W // 3:(3 * W) // 4 + 1] = 0; out["concave C"] = m
    out["3 % holes"] = (np.random.default_rng(5).random((H, W)) < 0.97).astype(np.uint8)
    out["lattice of zero pixels"] = ((xx % 7 != 0) | (yy % 5 != 0)).astype(np.uint8)
    out["box of one column"] = rect(3, H - 4, W // 2 + 1, W // 2 + 1)
    out["box of one pixel"] = rect(H - 2, H - 2, W - 3, W - 3)
    return out


@pytest.fixture(scope="module")
def cases():
    """(H, W) -> name -> (mask, d_in float32, d_in 16.16, max d_out), computed once and left unchanged."""
    out = {}
    rng = np.random.default_rng(77)
    for H, W in SHAPES:
        masks = _shape_masks(H, W)
        if (H, W) in ((96, 128), (150, 333)):
            masks.update({f"window kind {k}": _window_case(rng, H, W, k) for k in range(6)})
        if (H, W) == (131, 258):
            masks.update(_hard_masks(H, W))
        per = out[(H, W)] = {}
        for name, m in masks.items():
            if m.sum() == 0:
                m[H // 2, W // 2] = 1
            m.setflags(write=False)
            d, fix = O.distance_transform(m, 5, return_fix=True)
            d.setflags(write=False)
            per[name] = (m, d, fix.max(), O.distance_transform(1 - m, 5).max())
    return out


def _run(sel, masks):
    H, W = masks[0].shape
    depth = torch.full((len(masks), H, W), 0.5, dtype=torch.float32).cuda()
    maps, _, _ = sel.score_maps(torch.from_numpy(np.stack(masks)).cuda(), depth)
    return maps["distance_map"].cpu().numpy()


def _check(sel, per, names):
    got = _run(sel, [per[n][0] for n in names])
    searched = 0
    for i, n in enumerate(names):
        m, d_in, fix_max, mo_ref = per[n]
        mi, mo, _ = sel.dt_maxima(i)
        print(f"{n}: {int((got[i] != d_in).sum())} mismatches, max d_in {mi} / {d_in.max()}, max d_out {mo} / {mo_ref}")
        np.testing.assert_array_equal(got[i], d_in, err_msg=n)
        assert mi == np.float32(fix_max) * SCALE and mi == d_in.max(), n
        assert mo == mo_ref, n
        searched += sel.dt_form(i)[0]
    return searched


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_mask_of_a_shape_in_one_batch(sel, cases, shape):
    per = cases[shape]
    names = list(per)
    e_classes = set()
    for n in names:
        xs = np.nonzero(per[n][0])[1]
        e_classes.add(next(e for e in (4, 8, 16, 32, 64) if 64 * e >= xs.max() - (xs.min() & ~3) + 1))
    want = {128: {4}, 258: {4, 8}, 333: {4, 8}, 520: {4, 8, 16}, 1030: {4, 8, 16, 32}, 2048: {4, 8, 16, 32}, 2052: {4, 8, 16, 32, 64}}
    assert e_classes == want[shape[1]], "a span of every E class the width has room for"
    assert _check(sel, per, names) == len(names)   # every frame took the search
    assert sel.dt_search_form() == (6 if shape[1] <= 2048 else 5)


@pytest.mark.parametrize("shape", [(96, 128), (150, 333), (24, 2048)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_frames(sel, cases, shape):
    per = cases[shape]
    for n in [n for n in per if n.startswith(("span", "box of 1 rows", "box of 2 rows", "ring", "full-width", "leaf in the"))]:
        assert _check(sel, per, [n]) == 1
        assert sel.dt_search_form() == 6


def test_batch_of_nine_with_an_empty_mask_and_one_without_a_zero_pixel(sel, cases):
    H, W = 40, 520
    per = dict(cases[(H, W)])
    for name, m in (("empty", np.zeros((H, W), np.uint8)), ("full", np.ones((H, W), np.uint8))):
        d, fix = O.distance_transform(m, 5, return_fix=True)
        per[name] = (m, d, fix.max(), O.distance_transform(1 - m, 5).max())
    names = ["ring", "full", "3 % holes", "concave C", "empty", "box of one column", "full-width band", "box of 3 rows",
             "lattice of zero pixels"]
    got = _run(sel, [per[n][0] for n in names])
    assert sel.dt_search_form() == 6
    for i, n in enumerate(names):
        np.testing.assert_array_equal(got[i], per[n][1], err_msg=n)
        mi, mo, _ = sel.dt_maxima(i)
        assert mi == per[n][1].max(), n
        assert mo == per[n][3], n
        assert sel.dt_form(i)[0] == (n not in ("empty", "full")), n   # those two keep the sweeps, their neighbours take form 6


def test_stale_workspace_a_large_leaf_then_a_small_one(sel, cases):
    per = cases[(96, 128)]
    for n in ("3 % holes", "box of one pixel", "ring", "box of 1 rows", "leaf on the left border", "box of one column"):
        assert _check(sel, per, [n]) == 1
        assert sel.dt_search_form() == 6


def test_a_retired_form_number_is_ignored(cases):
    """LG_DT_SEARCH_ALGO=3 named the two-level search, which the library no longer has: the value leaves the default, a batch
    this small takes form 1, and the results are the oracle's."""
    s3 = _selector("3")
    assert _check(s3, cases[(40, 520)], ["ring", "concave C", "3 % holes"]) == 3
    assert s3.dt_search_form() == 1


@pytest.mark.parametrize("algo", ["5", "6"])
def test_forms_5_and_6_on_a_frame_lower_than_sixteen_rows_take_form_1(algo):
    """The seed rows of form 5 and the row registers of form 6 need the room of sixteen rows and columns."""
    H, W = 12, 40
    per = {}
    for n, m in _shape_masks(H, W).items():
        if n in ("ring", "3 % holes", "lattice of zero pixels", "leaf in the last corner", "box of 2 rows"):
            d, fix = O.distance_transform(m, 5, return_fix=True)
            per[n] = (m, d, fix.max(), O.distance_transform(1 - m, 5).max())
    assert len(per) == 5
    s = _selector(algo)
    assert _check(s, per, list(per)) == 5
    assert s.dt_search_form() == 1
