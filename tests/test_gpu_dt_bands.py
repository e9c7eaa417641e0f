"""Form 5 of the sweep-free distance transform (LG_DT_SEARCH_ALGO=5): pairs of adjacent rows every P rows by the bounded row
search (lg_dtseed_kernel<P>), the rows between two pairs by the 5 x 5 chamfer stencil run downwards and upwards in
registers (lg_dtband_kernel<P, E>; the identities: tests/test_dt_band_math.py).  Every built P -- and both column counts per
lane -- must give the oracle's two-pass transform bit for bit: distance_map, max d_in and max d_out.  The shapes are the
smallest that reach every path: widths that are no multiple of 4 (the scalar loads and stores) and multiples of 4 (the vector
ones), more than one wave tile across (the overlap seams: 200 columns per tile at P = 16, E = 4, 136 at P = 32, 72 at P = 16, E = 2), leaves lower than a band,
bands cut by the window's and the frame's last rows."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

FORMS = {"p12": (12, 4), "p16": (16, 4), "p24": (24, 4), "p32": (32, 4), "p16_e2": (16, 2), "p12_e2": (12, 2)}
SHAPES = [(96, 128), (150, 333), (131, 258), (200, 520), (300, 1030)]


@pytest.fixture(scope="module")
def sels():
    import leafgrasp_amd as L

    assert torch.cuda.is_available()
    out = {}
    for name, (p, e) in FORMS.items():
        env = {"LG_DT_SEARCH": "1", "LG_DT_SEARCH_ALGO": "5", "LG_DT_BAND_P": str(p), "LG_DT_BAND_E": str(e)}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:   # the options are read when a handle is created
            out[name] = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
            out[name].set_camera_params(O.synthetic_scene(64, 64, 0)[2])
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return out


def _window_case(rng, H, W, kind):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)

    def blob(cx, cy, a, b, ang):
        t = np.deg2rad(ang)
        u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
        v = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        return (u / a) ** 2 + (v / b) ** 2 <= 1.0

    if kind == 0:      # one small leaf anywhere (also hanging over the frame border)
        m |= blob(rng.uniform(-10, W + 10), rng.uniform(-10, H + 10), rng.uniform(5, W / 4), rng.uniform(4, H / 4), rng.uniform(0, 180))
    elif kind == 1:    # two far components: the window spans both, the gap rows / columns have no leaf pixel
        m |= blob(rng.uniform(0, W / 3), rng.uniform(0, H / 3), rng.uniform(3, 20), rng.uniform(3, 20), rng.uniform(0, 180))
        m |= blob(rng.uniform(2 * W / 3, W), rng.uniform(2 * H / 3, H), rng.uniform(3, 20), rng.uniform(3, 20), rng.uniform(0, 180))
    elif kind == 2:    # ring
        r = np.hypot(yy - rng.uniform(H / 3, 2 * H / 3), xx - rng.uniform(W / 3, 2 * W / 3))
        r0 = rng.uniform(6, min(H, W) / 3)
        m |= (r < r0) & (r > r0 * rng.uniform(0.3, 0.8))
    elif kind == 3:    # single pixels / thin lines (corners included)
        for _ in range(int(rng.integers(1, 4))):
            m[int(rng.integers(H)), int(rng.integers(W))] = 1
        if rng.random() < 0.5:
            m[int(rng.integers(H)), :] = 1
        if rng.random() < 0.3:
            m[0, 0] = 1
        if rng.random() < 0.3:
            m[H - 1, W - 1] = 1
    elif kind == 4:    # concave "C"
        m[H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
        m[H // 3:2 * H // 3, W // 3:3 * W // 4] = 0
    else:              # leaf touching one frame border
        side = int(rng.integers(4))
        cx = (0, W - 1, rng.uniform(0, W), rng.uniform(0, W))[side]
        cy = (rng.uniform(0, H), rng.uniform(0, H), 0, H - 1)[side]
        m |= blob(cx, cy, rng.uniform(5, W / 5), rng.uniform(5, H / 5), rng.uniform(0, 180))
    return m.astype(np.uint8)


def _hard_masks(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = H // 2, W // 2
    out = {}
    m = np.ones((H, W), np.uint8); m[(2 * H) // 3 + 4, (4 * W) // 5 - 5] = 0; out["one zero pixel inside"] = m
    m = np.ones((H, W), np.uint8); m[0, 0] = 0; out["one zero pixel, first corner"] = m
    m = np.ones((H, W), np.uint8); m[H - 1, W - 1] = 0; out["one zero pixel, last corner"] = m
    m = np.zeros((H, W), np.uint8); m[H // 5:(4 * H) // 5, :] = 1; out["full-width band"] = m
    m = np.zeros((H, W), np.uint8); m[:, W // 5:(3 * W) // 4] = 1; out["full-height band"] = m
    m = np.ones((H, W), np.uint8); m[:, 0] = 0; out["all but the first column"] = m
    m = np.ones((H, W), np.uint8); m[H - 1, :] = 0; out["all but the last row"] = m
    out["diagonal strip"] = (np.abs((yy - cy) - 0.35 * (xx - cx)) < 23).astype(np.uint8)
    out["steep strip"] = (np.abs((yy - cy) + 1.9 * (xx - cx)) < 60).astype(np.uint8)
    m = np.zeros((H, W), np.uint8); m[20:H - 20, 30:W - 30] = 1; m[20:H - 50, 60:W - 40:40] = 0; out["comb"] = m
    out["lattice of zero pixels"] = ((xx % 7 != 0) | (yy % 5 != 0)).astype(np.uint8)
    rng = np.random.default_rng(5)
    out["3 % holes"] = (rng.random((H, W)) < 0.97).astype(np.uint8)
    out["disc"] = (np.hypot(yy - cy, xx - cx) < 0.47 * H).astype(np.uint8)
    m = np.zeros((H, W), np.uint8); m[H // 2 + 3:H // 2 + 8, 40:W - 70] = 1; out["leaf lower than one band"] = m
    m = np.zeros((H, W), np.uint8); m[H // 2 + 1, 37:W - 11] = 1; out["leaf of one row"] = m
    m = np.zeros((H, W), np.uint8); m[0:H // 3, W // 4:W // 2 + 9] = 1; out["leaf from row 0"] = m
    m = np.zeros((H, W), np.uint8); m[H - H // 3:H, W // 3:W - 50] = 1; out["leaf to row H - 1"] = m
    m = np.zeros((H, W), np.uint8); m[H // 4:H // 2 + 5, 0:W // 3] = 1; out["leaf from column 0"] = m
    m = np.zeros((H, W), np.uint8); m[H // 3:H - 19, W - W // 3:W] = 1; out["leaf to column W - 1"] = m
    return out


@pytest.fixture(scope="module")
def cases():
    """name -> (mask, d_in, max d_out), computed once and left unchanged."""
    out = {}

    def add(name, m):
        m.setflags(write=False)
        d = O.distance_transform(m, 5)
        d.setflags(write=False)
        out[name] = (m, d, O.distance_transform(1 - m, 5).max())
    rng = np.random.default_rng(77)
    for si, (H, W) in enumerate(SHAPES):
        for kind in range(6):
            m = _window_case(rng, H, W, kind)
            if m.sum() == 0:
                m[H // 2, W // 2] = 1
            add(f"window {H}x{W} kind {kind}", m)
    for H, W in ((200, 520), (131, 258)):
        for name, m in _hard_masks(H, W).items():
            add(f"hard {H}x{W} {name}", m)
    H, W = 200, 520
    add(f"hard {H}x{W} empty", np.zeros((H, W), np.uint8))
    add(f"hard {H}x{W} full", np.ones((H, W), np.uint8))
    return out


def _check(sel, names, cases, batched):
    masks = [cases[n][0] for n in names]
    H, W = masks[0].shape
    depth = np.full((H, W), 0.5, np.float32)
    if batched:
        maps, _, _ = sel.score_maps(torch.from_numpy(np.stack(masks)).cuda(), torch.from_numpy(np.stack([depth] * len(masks))).cuda())
        got = maps["distance_map"].cpu().numpy()
    searched = 0
    for i, n in enumerate(names):
        m, d_in, mo_ref = cases[n]
        if not batched:
            maps, _, _ = sel.score_maps(torch.from_numpy(np.array(m)).cuda(), torch.from_numpy(depth).cuda())
        g = got[i] if batched else maps["distance_map"].cpu().numpy()
        f = i if batched else 0
        bad = int((g != d_in).sum())
        mi, mo, _ = sel.dt_maxima(f)
        print(f"{n}: {bad} mismatches, max d_in {mi} / {d_in.max()}, max d_out {mo} / {mo_ref}")
        np.testing.assert_array_equal(g, d_in, err_msg=n)
        assert mi == d_in.max(), n
        assert mo == mo_ref, n
        searched += sel.dt_form(f)[0]
    return searched


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", list(FORMS))
def test_windowed_cases(sels, cases, form, shape):
    names = [n for n in cases if n.startswith(f"window {shape[0]}x{shape[1]} ")]
    assert len(names) == 6
    assert _check(sels[form], names, cases, batched=False) == 6   # every one took the search


@pytest.mark.parametrize("shape", [(200, 520), (131, 258)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", list(FORMS))
def test_hard_masks(sels, cases, form, shape):
    names = [n for n in cases if n.startswith(f"hard {shape[0]}x{shape[1]} ") and not n.endswith((" empty", " full"))]
    assert len(names) == 19
    assert _check(sels[form], names, cases, batched=False) == 19


@pytest.mark.parametrize("nb", [1, 9, 17])
@pytest.mark.parametrize("form", list(FORMS))
def test_batches_mixing_the_masks_with_an_empty_and_a_full_one(sels, cases, form, nb):
    hard = [n for n in cases if n.startswith("hard 200x520 ")]
    pick = {1: ["hard 200x520 comb"], 9: hard[12:19] + hard[-2:], 17: hard[:13] + hard[-2:] + hard[13:15]}[nb]
    assert len(pick) == nb
    searched = _check(sels[form], pick, cases, batched=True)
    assert searched == nb - (0 if nb == 1 else 2)   # the empty and the full mask go through the sweeps
