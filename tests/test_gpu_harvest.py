"""lg_harvest_patches against plain NumPy slices, bit for bit, at the frame's edges (-m gpu).

The kernel copies 32x32 windows of depth, mask and seven score planes, rotates them by rot & 3 quarter turns and flags
what the reference's _extract_patches (scripts/utils/ml_grasp_optimizer/data_collector.py:91-173) refuses.  A window is
inside the frame iff 16 <= x <= W-16 and 16 <= y <= H-16 (the slices of :103-104 are full there; the far edge is
inclusive, pinned by tests/golden/collector_edges.npz).  Expected flags: 1 non-finite depth, 2 empty mask window,
4 non-finite score, 8 ALONE for a window outside the frame, whose output rows stay untouched.

torch.rot90 (the reference's _rotate_tensor) takes k modulo 4, and so does np.rot90; the kernel's rot & 3 is the same
residue for negative k in two's complement, as Python's k & 3 is.  So np.rot90(., rot & 3) is the expected rotation for
every rot in -5..9."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import collector_cases as CC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(32, 32), (33, 47), (67, 130), (160, 224)]
SENT, FSENT = np.float32(-77.25), -99
I32MAX, I32MIN = 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope="module")
def collector(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import leafgrasp_amd as L

    return L.EnhancedGraspDataCollector(patch_size=32, resume=False, data_dir=str(tmp_path_factory.mktemp("lg_harvest")),
                                        device="cuda:0")


def _frame(H, W, seed):
    """depth, mask and seven DISTINCT random planes.  The mask holds the two side columns (every window on the left and
    right edge lines is accepted), half of the top and bottom rows on wide frames, and sparse specks: many interior
    windows are empty."""
    rng = np.random.default_rng(seed)
    depth = (rng.random((H, W), dtype=np.float32) + np.float32(0.25))
    planes = [rng.standard_normal((H, W)).astype(np.float32) + np.float32(10 * (c + 1)) for c in range(7)]
    mask = np.zeros((H, W), np.uint8)
    mask[:, 0] = mask[:, W - 1] = 1
    if W >= 100:
        mask[0, W // 2:] = 1
        mask[H - 1, :W // 2] = 1
        mask[rng.random((H, W)) > 0.9985] = 3            # any non-zero value is leaf
    return depth, mask, planes


def _points(H, W, seed):
    rng = np.random.default_rng(seed + 1)
    xs, ys = range(16, W - 15), range(16, H - 15)                    # valid centres: 16..W-16, 16..H-16
    pts = []
    for c in ((16, 16), (W - 16, 16), (16, H - 16), (W - 16, H - 16)):
        pts += [c] * 15                                              # one per rot in -5..9 (at 32x32 the only centre)
    pts += [(x, y) for y in (16, H - 16) for x in xs] + [(x, y) for x in (16, W - 16) for y in ys]   # the four edge lines
    pts += [(x, y) for y in (15, H - 15) for x in range(15, W - 14)] + [(x, y) for x in (15, W - 15) for y in range(15, H - 14)]
    pts += [(0, 0), (W - 1, H - 1), (-1, 20), (20, -1), (-16, -16), (W, H), (W + 16, 20), (20, H + 16), (-1000, 40), (40, 10 ** 6),
            (I32MAX, 20), (20, I32MAX), (I32MIN, 20), (20, I32MIN), (I32MAX, I32MAX), (I32MIN, I32MIN), (I32MAX - 15, 16),
            (16, I32MAX - 15), (I32MAX - 16, I32MAX - 16), (W - 16, I32MIN + 16)]
    pts += [(int(rng.integers(16, W - 15)), int(rng.integers(16, H - 15))) for _ in range(60)]
    rots = [k for _ in range(4) for k in range(-5, 10)] + [int(r) for r in rng.integers(-5, 10, len(pts) - 60)]
    return pts, rots


def _expected(depth, mask, planes, pts, rots):
    H, W = mask.shape
    n = len(pts)
    od = np.full((n, 32, 32), SENT, np.float32)
    om = np.full((n, 32, 32), SENT, np.float32)
    osc = np.full((n, 7, 32, 32), SENT, np.float32)
    fl = np.zeros(n, np.int32)
    for i, (x, y) in enumerate(pts):
        if not (16 <= x <= W - 16 and 16 <= y <= H - 16):
            fl[i] = 8
            continue
        k = (rots[i] & 3) if rots is not None else 0
        sl = (slice(y - 16, y + 16), slice(x - 16, x + 16))
        d, m = depth[sl], (mask[sl] != 0).astype(np.float32)
        sc = np.stack([p[sl] for p in planes])
        fl[i] = 1 * (not np.isfinite(d).all()) + 2 * (not m.any()) + 4 * (not np.isfinite(sc).all())
        od[i], om[i], osc[i] = np.rot90(d, k), np.rot90(m, k), np.rot90(sc, k, axes=(-2, -1))
    return od, om, osc, fl


def _harvest(col, depth, mask, planes, pts, rots):
    """lg_harvest_patches through the C-ABI on sentinel-filled outputs."""
    from leafgrasp_amd._lib import LG_NUM_MAPS, check, lib

    H, W = mask.shape
    n = len(pts)
    dev = col.device
    d = torch.from_numpy(depth).to(dev)
    m = torch.from_numpy(mask).to(dev)
    pl = [torch.from_numpy(p).to(dev) for p in planes]
    xy = torch.tensor(pts, dtype=torch.int32, device=dev).reshape(n, 2).contiguous()
    rot = torch.tensor(rots, dtype=torch.int32, device=dev) if rots is not None else None
    od = torch.full((n, 32, 32), float(SENT), dtype=torch.float32, device=dev)
    om = torch.full((n, 32, 32), float(SENT), dtype=torch.float32, device=dev)
    osc = torch.full((n, 7, 32, 32), float(SENT), dtype=torch.float32, device=dev)
    fl = torch.full((n,), FSENT, dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * LG_NUM_MAPS)()
    for i, p in enumerate(pl):
        ptrs[i] = p.data_ptr()
    with torch.cuda.device(dev):
        check(col._h, lib.lg_harvest_patches(col._h, d.data_ptr(), m.data_ptr(), C.byref(ptrs), H, W, n, xy.data_ptr(),
                                             rot.data_ptr() if rot is not None else None, od.data_ptr(), om.data_ptr(),
                                             osc.data_ptr(), fl.data_ptr(), col._stream()), "lg_harvest_patches")
        torch.cuda.synchronize()
    return od.cpu().numpy(), om.cpu().numpy(), osc.cpu().numpy(), fl.cpu().numpy()


def _same_bits(got, exp, what):
    """Bit-exact, NaN payloads and signs included (the kernel copies)."""
    g, e = got.view(np.uint32), exp.view(np.uint32)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _check(col, depth, mask, planes, pts, rots, what):
    exp = _expected(depth, mask, planes, pts, rots)
    got = _harvest(col, depth, mask, planes, pts, rots)
    np.testing.assert_array_equal(got[3], exp[3], err_msg=f"{what}: flags")
    for g, e, name in zip(got[:3], exp[:3], ("depth", "mask", "scores")):
        _same_bits(g, e, f"{what}: {name}")              # rows of flag 8 still hold the sentinel
    return exp[3]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_harvest_windows_on_every_edge_line_and_outside(collector, shape):
    H, W = shape
    depth, mask, planes = _frame(H, W, 100 + H)
    pts, rots = _points(H, W, H)
    assert len(pts) == len(rots) and min(rots) == -5 and max(rots) == 9
    fl = _check(collector, depth, mask, planes, pts, rots, "rot")
    # the NumPy side first: the case list does what it says
    acc = [(p, r) for p, r, f in zip(pts, rots, fl) if f == 0]
    assert {0, 8} <= set(fl.tolist()) and (2 in fl or shape == (32, 32))
    assert any(x == 16 for (x, _), _ in acc) and any(x == W - 16 for (x, _), _ in acc)
    assert any(y == 16 for (_, y), _ in acc) and any(y == H - 16 for (_, y), _ in acc)
    assert {r & 3 for _, r in acc} == {0, 1, 2, 3} and {r for _, r in acc} >= set(range(-5, 10))
    ring = [(x, y) for (x, y) in pts if x in (15, W - 15) or y in (15, H - 15)]
    assert ring and all(f == 8 for p, f in zip(pts, fl) if p in set(ring))
    # rot = NULL: no rotation
    fl0 = _check(collector, depth, mask, planes, pts, None, "rot NULL")
    np.testing.assert_array_equal(fl0, fl)


def _poison_cases(H, W, seed):
    """(target, value, window centre, pixel) -- target 'd' or a plane index; the pixel sits at the window's corners
    (0,0) and (31,31), inside it, or one pixel outside it (where the frame has room)."""
    rng = np.random.default_rng(seed)
    vals = [np.float32(np.nan), -np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    assert [np.signbit(v) for v in vals] == [False, True, False, True]
    out, i = [], 0
    for target in ["d"] + list(range(7)):
        for pos in ((0, 0), (31, 31), (13, 18), (-1, 5), (32, 7), (9, -1), (20, 32)):
            cx, cy = int(rng.integers(16, W - 15)), int(rng.integers(16, H - 15))
            if pos[0] == -1:
                cy = min(H - 16, cy + 1)
            if pos[1] == -1:
                cx = min(W - 16, cx + 1)
            py, px = cy - 16 + pos[0], cx - 16 + pos[1]
            if not (0 <= py < H and 0 <= px < W):
                continue                                  # a 32-px-high (wide) frame has no pixel outside its window
            out.append((target, vals[i % 4], (cx, cy), (py, px), pos))
            i += 1
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_harvest_single_non_finite_pixels_and_combined_flags(collector, shape):
    H, W = shape
    depth, mask, planes = _frame(H, W, 200 + H)
    mask[:] = 1                                           # the mask bit is not the subject here (until the combinations)
    rng = np.random.default_rng(H * W)
    seen, outside_ok = set(), 0
    seen |= set(_check(collector, depth, mask, planes, [(16, 16), (W - 16, H - 16)], [-1, 6], "clean").tolist())
    cases = _poison_cases(H, W, H + W)
    assert {c[0] for c in cases} == {"d", 0, 1, 2, 3, 4, 5, 6} and {c[4] for c in cases} >= {(0, 0), (31, 31), (13, 18)}
    for target, val, (cx, cy), (py, px), pos in cases:
        d, pl = depth.copy(), [p.copy() for p in planes]
        (d if target == "d" else pl[target])[py, px] = val
        pts = [(cx, cy), (cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1), (px + 16, py + 16), (px - 15, py - 15),
               (px + 17, py + 16), (px + 16, py + 17), (px - 16, py - 15), (px - 15, py - 16)]
        pts += [(int(rng.integers(16, W - 15)), int(rng.integers(16, H - 15))) for _ in range(12)]
        rots = [int(r) for r in rng.integers(-5, 10, len(pts))]
        fl = _check(collector, d, mask, pl, pts, rots, f"{target} {val} at {pos}")
        want = 1 if target == "d" else 4
        inside = 0 <= pos[0] < 32 and 0 <= pos[1] < 32
        assert fl[0] == (want if inside else 0), (target, pos, fl[0])
        outside_ok += not inside
        seen |= set(fl.tolist())
    assert outside_ok > 0 or H == 32 or W == 32
    # combinations: empty mask (2) with NaN depth (1) and / or an infinite score (4)
    empty = np.zeros_like(mask)
    c = (W // 2 if W > 32 else 16, H // 2 if H > 32 else 16)
    pts = [c, (16, 16), (W - 16, H - 16), (15, 15)]
    for bad_d, bad_s, want in ((False, False, 2), (True, False, 3), (False, True, 6), (True, True, 7)):
        d, pl = depth.copy(), [p.copy() for p in planes]
        if bad_d:
            d[c[1] - 16, c[0] - 16] = np.float32(np.nan)
        if bad_s:
            pl[6][c[1] + 15, c[0] + 15] = np.float32(-np.inf)
        fl = _check(collector, d, empty, pl, pts, [1, 2, 3, 0], f"combined {want}")
        assert fl[0] == want and fl[3] == 8
        seen |= set(fl.tolist())
    d, pl = depth.copy(), [p.copy() for p in planes]     # non-finite depth AND score on the leaf: 5
    d[c[1], c[0]] = np.float32(np.inf)
    pl[0][c[1], c[0]] = -np.float32(np.nan)
    fl = _check(collector, d, mask, pl, pts, None, "combined 5")
    assert fl[0] == 5
    seen.add(5)
    assert {0, 1, 2, 4, 8, 3, 5, 6, 7} <= seen, seen


def test_mirror_methods_reproduce_the_reference_at_frame_edges(collector):
    """EnhancedGraspDataCollector._extract_patches / _check_boundaries against tests/golden/collector_edges.npz: the
    REFERENCE's answers at (16,16), (W-16,16), (16,H-16), (W-16,H-16), one pixel past each edge line, the corners."""
    gold = np.load(os.path.join(HERE, "golden", "collector_edges.npz"))
    mask, depth, scores = CC.edges_scene()
    H, W = mask.shape
    mt, dt = torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(depth).cuda()
    sc = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in scores.items()}
    pts = [(int(x), int(y)) for x, y in gold["pts"]]
    np.testing.assert_array_equal([collector._check_boundaries(x, y, mask.shape, 16) for x, y in pts], gold["bounds_ok"])
    got = [collector._extract_patches(x, y, mt, dt, sc) for x, y in pts]
    np.testing.assert_array_equal(np.array([g is not None for g in got]), gold["ok"])
    assert gold["ok"][:4].all() and pts[3] == (W - 16, H - 16) and not gold["bounds_ok"][1:4].any()
    kept = [g for g in got if g is not None]
    np.testing.assert_array_equal(np.stack([g[0].numpy() for g in kept]), gold["depth"])
    np.testing.assert_array_equal(np.stack([g[1].numpy() for g in kept]), gold["mask_patches"])
    np.testing.assert_array_equal(np.stack([g[2].numpy() for g in kept]), gold["scores"])
