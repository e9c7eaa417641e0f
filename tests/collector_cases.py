"""Inputs shared by the collector's edge tests (test_collector_edges.py, test_contour_points_host.py,
test_gpu_harvest.py, test_gpu_negative_regions.py, test_gpu_collect_sample.py) and by
tests/golden/make_golden_collector.py: the 67x130 scene whose leaf reaches every corner and edge of the frame, the masks
the negative regions and the contour are held on, and the NumPy replay of the reference's collect_sample
(scripts/utils/ml_grasp_optimizer/data_collector.py:175-348) on the oracle's helpers."""
import random

import numpy as np

from oracle import lg_oracle as O

EDGE_H, EDGE_W, EDGE_SEED = 67, 130, 5


def ellipse(H, W, cx, cy, a, b):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((xx - cx) / float(a)) ** 2 + ((yy - cy) / float(b)) ** 2 <= 1.0).astype(np.uint8)


def edges_mask(H=EDGE_H, W=EDGE_W):
    """Leaf ellipses in the four corners, on the middle of the four edges and at the centre: every 32x32 window that
    touches a corner or the middle of an edge holds leaf pixels."""
    m = ellipse(H, W, W // 2, H // 2, 22, 11)
    for cx, cy in ((4, 4), (W - 5, 4), (4, H - 5), (W - 5, H - 5), (W // 2, 2), (W // 2, H - 3), (2, H // 2), (W - 3, H // 2),
                   (40, 3), (40, H - 4), (3, 40), (W - 4, 40)):
        m |= ellipse(H, W, cx, cy, 9, 7)
    return m


def edges_scene():
    """mask u8, depth f32 and the oracle's score planes (float32) of the 67x130 edge scene."""
    mask = edges_mask()
    depth, scores = scene_scores(mask, EDGE_SEED)
    return mask, depth, scores


def edges_points(H=EDGE_H, W=EDGE_W):
    """The four extreme centres (accepted by the slices, the two far ones refused by _check_boundaries), one pixel past
    each edge line, the frame's corners, interior points."""
    return [(16, 16), (W - 16, 16), (16, H - 16), (W - 16, H - 16),
            (W - 15, 40), (40, H - 15), (15, 40), (40, 15), (0, 0), (W - 1, H - 1),
            (W // 2, H // 2), (50, 30), (80, 36), (W - 17, H - 17), (17, 17)]


# ------------------------------------------------------------------------------------------------ negative regions
def region_masks(H, W):
    """name -> u8 mask.  Bars sit in the bottom quarter (rows >= int(0.75 H)), where the stem erosion looks."""
    q = int(0.75 * H)
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8)}
    m = np.zeros((H, W), np.uint8)                       # touches the bottom row and both sides
    m[H // 3:, :] = ellipse(H, W, (W - 1) / 2.0, H - 1, 0.75 * W, 0.6 * H)[H // 3:, :]
    m[H - 1, :] = 1
    out["bottom_sides"] = m
    for wpx in (5, 9):                                   # a vertical bar exactly wpx wide, inside the bottom quarter
        m = np.zeros((H, W), np.uint8)
        x0 = min(max(1, W // 3), max(0, W - wpx - 1))
        m[q:H, x0:x0 + wpx] = 1
        out[f"bar{wpx}"] = m
    m = np.zeros((H, W), np.uint8)                       # a bar across row int(0.75 H): only the rows >= q may survive
    m[max(0, q - 8):min(H, q + 12), max(0, W // 5):max(W // 5 + 1, W - W // 5)] = 1
    out["straddle"] = m
    if W > 64:                                           # a blob over the column 63 | 64 boundary of the 64-wide tiles
        m = np.zeros((H, W), np.uint8)
        m[max(0, q - 3):H, 50:min(W, 80)] = 1
        m[max(0, q - 3), 50] = m[H - 1, 50] = 0
        m[q + 1, 63] = 0                                  # a hole next to the boundary: erodes columns on both sides
        out["cross64"] = m
    m = np.zeros((H, W), np.uint8)                       # rectangle: the ridge of its transform is a plateau
    y0, x0 = max(0, H // 8), max(0, W // 8)
    m[y0:y0 + max(3, H // 2) // 2 * 2 + 1, x0:max(x0 + 3, W - W // 8)] = 1
    out["ridge"] = m
    return out


def tip_plane(mask, dist):
    """(cv2.dilate(dist, ones(5,5)) == dist) & (mask > 0) over the whole frame; cv2's dilation ignores the border."""
    H, W = mask.shape
    pad = np.full((H + 4, W + 4), -np.inf, np.float32)
    pad[2:-2, 2:-2] = dist
    mx = np.max(np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)]), axis=0)
    return ((mx == dist) & (mask > 0)).astype(np.uint8)


def erode5(src, first_row=0):
    """One cv2.erode by the 5x5 MORPH_ELLIPSE (rows -2 / +2: the centre column; rows -1..1: five columns), written
    without the oracle's dilate: a pixel survives iff every element position INSIDE the frame is set."""
    H, W = src.shape
    s = (src != 0)
    s[:first_row] = False
    keep = np.ones((H, W), bool)
    for dy in range(-2, 3):
        r = 0 if abs(dy) == 2 else 2
        for dx in range(-r, r + 1):
            sh = np.ones((H, W), bool)                   # outside the frame: does not erode
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            if ys.start < ys.stop and xs.start < xs.stop:
                sh[yd, xd] = s[ys, xs]
            keep &= sh
    return keep.astype(np.uint8)


def stem_plane(mask):
    H = mask.shape[0]
    return erode5(erode5(mask, int(0.75 * H)))


# ------------------------------------------------------------------------------------------------ contour
def contour_masks(H, W):
    """name -> u8 mask for the contour trace."""
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8)}
    m = np.zeros((H, W), np.uint8); m[H // 2, W // 3] = 1
    out["pixel"] = m
    m = np.zeros((H, W), np.uint8); m[H // 3, 2:W - 2] = 1                    # the contour doubles back along the line
    out["line"] = m
    m = np.zeros((H, W), np.uint8); m[2:6, 3:8] = 1; m[H - 7:H - 3, W - 9:W - 4] = 1
    out["equal_pair"] = m                                                      # two 4x5 rectangles: equal contour area
    m = np.zeros((H, W), np.uint8); m[1, 1] = 1; m[3, 5:9] = 1; m[H - 2, W - 2] = 1; m[5:9, 2] = 1
    out["area0"] = m                                                           # pixels and 1-px lines: every area is 0
    m = np.zeros((H, W), np.uint8)                                             # comb: 1-px teeth, 1-px gaps
    m[H - 2, 1:W - 1] = 1
    m[1:H - 2, 1:W - 1:2] = 1
    out["comb"] = m
    m = ellipse(H, W, W * 0.5, H * 0.5, W * 0.4, H * 0.35)
    m[H // 2, :] = 1                                                            # spikes to both sides of the frame
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = 1
    out["spiked"] = m
    return out


def random_contour_masks():
    """The 120 masks of tests/test_host_contour.py's generator (same rng, same draws for the shapes and the masks; the
    probe draws of that file come after each mask and are consumed here the same way)."""
    rng = np.random.default_rng(11)
    out = []
    for case in range(120):
        H, W = int(rng.integers(3, 90)), int(rng.integers(3, 200))
        kind = case % 5
        if kind == 0:
            m = (rng.random((H, W)) > 0.6)
        elif kind == 1:
            m = (rng.random((H, W)) > 0.97)
        elif kind == 2:
            yy, xx = np.mgrid[0:H, 0:W]
            m = ((xx - W * 0.5) / (W * 0.4)) ** 2 + ((yy - H * 0.5) / (H * 0.35)) ** 2 <= 1
            m &= ~(((xx - W * 0.5) / (W * 0.15)) ** 2 + ((yy - H * 0.5) / (H * 0.12)) ** 2 <= 1)
            m[0, :3] = True
        elif kind == 3:
            m = np.ones((H, W), bool)
        else:
            m = np.zeros((H, W), bool)
            m[H // 3: H // 3 + max(1, H // 4), :] = rng.random(
                (max(1, H // 4) if H // 3 + max(1, H // 4) <= H else H - H // 3, W)) > 0.3
        m = m.astype(np.uint8)
        if m.any():
            for _ in range(10):
                rng.integers(0, W), rng.integers(0, H)
        for _ in range(20):
            rng.integers(0, W), rng.integers(0, H)
        out.append(m)
    return out


def pack_bits(m):
    """u8 [H,W] -> the product's bit rows: uint64 [H, WW], bit x & 63 of word x >> 6."""
    H, W = m.shape
    WW = (W + 63) // 64
    padded = np.zeros((H, WW * 64), np.uint8)
    padded[:, :W] = m != 0
    return np.packbits(padded.reshape(H, WW, 64), axis=2, bitorder="little").view(np.uint64).reshape(H, WW).copy()


# ------------------------------------------------------------------------------------------------ collect_sample
def collect_scene_masks(H=160, W=224):
    """The leaf collect_sample runs on (an ellipse that reaches into the bottom quarter, with a 1-pixel spike) and a
    DIFFERENT leaf whose distance transform stands in for scores['distance_map'] in the tip-source test."""
    leaf = ellipse(H, W, 110, 125, 70, 30)
    leaf[122, 170:220] = 1
    other = ellipse(H, W, 80, 100, 40, 55)
    return leaf, other


def scene_scores(mask, seed):
    """depth f32 and the oracle's score planes (float32) for `mask` on the synthetic scene's depth."""
    H, W = mask.shape
    _, depth, P = O.synthetic_scene(H, W, seed)
    ref = O.RefGraspPointSelector()
    ref.set_camera_params(P)
    return depth, {k: np.asarray(v, dtype=np.float32) for k, v in ref._calculate_all_scores(mask, depth).items()}


def corner_scene(H=EDGE_H, W=EDGE_W):
    """A small disc centred on (W-16, H-16): the only tip point is that centre, the last pixel whose window the slices
    accept and _check_boundaries refuses; no stem or edge points."""
    mask = ellipse(H, W, W - 16, H - 16, 5, 5)
    depth, scores = scene_scores(mask, EDGE_SEED)
    return mask, depth, scores


def replay_collect_sample(mask, depth, scores, point, total, seed):
    """The reference's collect_sample (:175-348) on the oracle's helpers with `random` seeded like the product run.
    -> list of (patches, grasp_point, total_score, label, source) or None when the positive is refused; source is
    'pos', 'aug', 'tip', 'stem' or 'edge'.  Tip points come from the MASK (_get_tip_points :425 recomputes the
    transform), score patches from the planes as handed in."""
    gx, gy = point
    if not O.collector_check_boundaries(gx, gy, mask.shape, 16):          # :203, the positive only
        return None
    random.seed(seed)
    p0 = O.collector_extract_patches(gx, gy, mask, depth, scores)
    if p0 is None:
        return None
    exp = [(p0, (gx, gy), total, 1, "pos")]
    for k, ang in enumerate((90, 180, 270), start=1):
        random.uniform(0.01, 0.02)
        exp.append((O.collector_extract_patches(gx, gy, mask, depth, scores, k=k),
                    O.collector_rotate_point((gx, gy), ang, 32), total * random.uniform(0.95, 1.0), 1, "aug"))
    lists = (("tip", O.collector_tip_points(mask)), ("stem", O.collector_stem_points(mask)),
             ("edge", O.collector_edge_points(mask)))
    collected = attempts = 0
    while collected < 3 and attempts < 10:
        neg = []
        for name, lst in lists:
            if lst:
                neg.extend((name, p) for p in random.sample(lst, 1))
        for name, (x, y) in neg:
            if collected >= 3:
                break
            p = O.collector_extract_patches(x, y, mask, depth, scores)    # :332: no _check_boundaries
            if p is not None:
                exp.append((p, (x, y), 0.0, 0, name))
                collected += 1
        attempts += 1
    return exp
