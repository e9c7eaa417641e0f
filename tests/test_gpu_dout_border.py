"""max d_out on the frame border lines (lg_dout_border_kernel: the profile of the leaf seen from a border line, then the pruned
search lg_border_cand_min over the line's candidates) against the oracle's two-pass transform, bit for bit.  Every case names
the border lines it is there for; the test reads the sweep window the device reports and asserts that those lines lay outside
it -- the lines the kernel walks -- so no case passes on the sweeps alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

SHAPES = [(96, 320), (48, 704), (704, 128)]


def _ellipse(H, W, x0, x1, y0, y1):
    yy, xx = np.mgrid[0:H, 0:W]
    cx, cy, a, b = (x0 + x1) / 2.0, (y0 + y1) / 2.0, (x1 - x0) / 2.0 + 0.3, (y1 - y0) / 2.0 + 0.3
    m = (((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0)
    m[y0:y1 + 1, x0] |= (np.arange(y0, y1 + 1) % 7 == 3)   # ragged: the profile is not convex
    m[y0, x0:x1 + 1] |= (np.arange(x0, x1 + 1) % 11 == 5)
    return m.astype(np.uint8)


def _cases(H, W):
    """name -> (mask, border lines that must lie outside the window)"""
    out = {}
    wide = W >= 192                        # room for 64 clear columns on both sides
    cx0, cx1 = 64 + 3, (W - 64 - 5 if wide else W - 6)
    cy0, cy1 = 16 + 2, H - 16 - 3
    # the right line lies outside only when the window's last sweep wave (256 columns) ends before it: never in a frame of up to
    # 256 columns
    out["clear of every border"] = (_ellipse(H, W, cx0, cx1, cy0, cy1), {"top", "bottom", "left"})
    out["against the top"] = (_ellipse(H, W, cx0, cx1, 0, cy1 - cy0), {"bottom", "left"})
    out["against the bottom"] = (_ellipse(H, W, cx0, cx1, H - 1 - (cy1 - cy0), H - 1), {"top", "left"})
    out["against the left"] = (_ellipse(H, W, 0, min(cx1 - cx0, 40), cy0, cy1), {"top", "bottom"} | ({"right"} if W > 256 else set()))
    out["against the right"] = (_ellipse(H, W, W - 1 - (cx1 - cx0), W - 1, cy0, cy1), {"top", "bottom"} | ({"left"} if wide else set()))
    if W > 300:   # a bounding box more than 256 wide: two rounds of candidates on the horizontal lines
        out["box wider than 256"] = (_ellipse(H, W, 10, W - 12, cy0, cy1), {"top", "bottom"})
        m = np.zeros((H, W), np.uint8)   # U open to the top: the maximum of the top line lies inside the span
        m[16:H - 19, 2:5] = 1; m[16:H - 19, W - 5:W - 2] = 1; m[H - 22:H - 19, 2:W - 2] = 1
        out["u open to the top"] = (m, {"top", "bottom"})
    if H > 300:   # more than 256 tall: several rounds on the vertical lines, many row chunks per word on the horizontal ones
        out["box taller than 256"] = (_ellipse(H, W, 70, W - 8, 30, H - 100), {"top", "bottom", "left"})
    m = np.zeros((H, W), np.uint8)       # U open to the left
    m[2:5, 64:W - 2] = 1; m[H - 5:H - 2, 64:W - 2] = 1; m[2:H - 2, W - 5:W - 2] = 1
    out["u open to the left"] = (m, {"left"})
    m = _ellipse(H, W, 66, 90, cy0, cy1) | _ellipse(H, W, 100, 125, cy0 + 3, cy1)
    if wide:
        m |= _ellipse(H, W, 170, min(W - 70, 260), cy0 + 1, cy1 - 2)
    out["components with empty columns between"] = (m, {"top", "bottom", "left"})
    m = np.zeros((H, W), np.uint8); m[H // 2 + 1, 100] = 1
    out["single pixel"] = (m, {"top", "bottom", "left"})
    m = np.zeros((H, W), np.uint8); m[H // 2 - 3, 70:W - 4] = 1
    out["leaf of one row"] = (m, {"top", "bottom", "left"})
    m = np.zeros((H, W), np.uint8); m[cy0:cy1 + 1, 101] = 1
    out["leaf of one column"] = (m, {"top", "bottom", "left"})
    return out


@pytest.fixture(scope="module")
def sel():
    import leafgrasp_amd as L

    assert torch.cuda.is_available()
    s = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    s.set_camera_params(O.synthetic_scene(64, 64, 0)[2])
    return s


@pytest.fixture(scope="module")
def cases():
    """(H, W) -> name -> (mask, lines, the oracle's max d_out), computed once and left unchanged"""
    out = {}
    for H, W in SHAPES:
        out[(H, W)] = {}
        for name, (m, lines) in _cases(H, W).items():
            m.setflags(write=False)
            out[(H, W)][name] = (m, frozenset(lines), O.distance_transform(1 - m, 5).max())
    return out


def _outside(win, H, W):
    x0, x1, y0, y1 = win
    return {s for s, o in (("top", y0 > 0), ("bottom", y1 < H), ("left", x0 > 0), ("right", x1 < W)) if o}


def _run(sel, masks):
    H, W = masks[0].shape
    depth = np.full((len(masks), H, W), 0.5, np.float32)
    sel.score_maps(torch.from_numpy(np.stack(masks)).cuda(), torch.from_numpy(depth).cuda())
    return [sel.dt_maxima(i) for i in range(len(masks))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_case_alone(sel, cases, shape):
    H, W = shape
    seen = set()
    for name, (m, lines, mo_ref) in cases[shape].items():
        _, mo, win = _run(sel, [np.array(m)])[0]
        outside = _outside(win, H, W)
        print(f"{H}x{W} {name}: max d_out {mo} / {mo_ref}, window {win}, outside {sorted(outside)}")
        assert lines <= outside, (name, win)
        assert mo == mo_ref, name
        seen |= outside
    assert seen == {"top", "bottom", "left"} | ({"right"} if W > 256 else set())


def test_batch_of_nine_with_an_empty_mask(sel, cases):
    H, W = 96, 320
    c = cases[(H, W)]
    names = ["clear of every border", "against the left", "u open to the top", "box wider than 256", "single pixel",
             "u open to the left", "components with empty columns between", "leaf of one column"]
    masks = [np.array(c[n][0]) for n in names]
    masks.insert(4, np.zeros((H, W), np.uint8))
    got = _run(sel, masks)
    refs = [c[n] for n in names]
    refs.insert(4, None)
    assert len(masks) == 9
    for i, (g, r) in enumerate(zip(got, refs)):
        if r is None:   # no source pixel: the window is the whole frame, no line is walked
            assert _outside(g[2], H, W) == set()
            assert g[1] == O.distance_transform(np.ones((H, W), np.uint8), 5).max()
            continue
        assert r[1] <= _outside(g[2], H, W), i
        assert g[1] == r[2], i
