"""Test-side reference of the collecting selector (lg_select_grasp_collect; scripts/utils/grasp_point_selector_bkp.py:73-169),
composed from the oracle's parts: the erosion by the complement identity over O.dilate / O.ellipse_se (the identity
O.collector_stem_points uses), RefGraspPointSelector._calculate_all_scores on the safe zone with flatness_map taken on depth *
the ORIGINAL mask, O.distance_transform(..., 5) for the tip penalty, and the variant's fusion.  The oracle is not edited."""
import math

import numpy as np

from oracle import lg_oracle as O

TIP_KEY = "tip_penalty"


def erode(mask, k=21, iterations=2):
    """cv2.erode(mask, ellipse(k, k), iterations=iterations): the ellipse is symmetric under a half turn, so one erosion is the
    complement of the dilation of the complement; O.dilate reads 0 outside the frame, so the frame border does not erode."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    se = O.ellipse_se(k)
    for _ in range(iterations):
        m = (1 - O.dilate(1 - m, se)).astype(np.uint8)
    return m


def tip_field_as_written(H, W, init_dist0=O.INIT_DIST0):
    """(d float32, fix uint32) of cv2.distanceTransform((~tip_area).astype(uint8), DIST_L2, 5): a 0 / 1 uint8 image inverted is
    255 or 254 everywhere -- no zero pixel, whatever the tip area (bkp:399-402)."""
    return O.distance_transform(np.full((H, W), 255, np.uint8), 5, return_fix=True, init_dist0=init_dist0)


def tip_penalty_as_written(safe, init_dist0=O.INIT_DIST0):
    """bkp:403-405 in float32 (the rules of the isolation plane, oracle lines 401-405): (1 - d / (max d + 1e-6)) * safe"""
    safe = np.asarray(safe, np.uint8)
    d, _ = tip_field_as_written(safe.shape[0], safe.shape[1], init_dist0)
    mx = np.float32(np.float32(d.max()) + np.float32(1e-6))
    return ((np.float32(1.0) - d / mx) * safe.astype(np.float32)).astype(np.float32)


def centroid(mask):
    """ImageProcessor.calculate_centroid (image_processor.py:49-54) + int(): (x, y), or None for an empty mask (int(nan) raises).
    Also the fractional parts of the two means, for the tests that keep clear of a knife edge."""
    ys, xs = np.nonzero(np.asarray(mask))
    if len(xs) == 0:
        return None, (math.nan, math.nan)
    mx, my = float(np.float32(xs.mean())), float(np.float32(ys.mean()))
    return (int(mx), int(my)), (mx - int(mx), my - int(my))


def compose(mask, depth, P, params=None, k=21, iterations=2, w_tip=0.1):
    """Everything lg_select_grasp_collect returns for one frame, as a dict: safe, scores (the seven planes + tip_penalty +
    traditional_score), valid, point, by_argmax, best_score (np.max of the fused plane), point_3d, pre_grasp, theta."""
    p = O.ref_params(params)
    mask = (np.asarray(mask) != 0).astype(np.uint8)
    depth = np.asarray(depth, np.float32)
    safe = erode(mask, k, iterations)
    ref = O.RefGraspPointSelector(params=p)
    ref.set_camera_params(P)
    sc = ref._calculate_all_scores(safe, depth)                                             # bkp:85-93 on the safe zone
    sc["flatness_map"] = O.flatness_map(depth * mask.astype(np.float32), p.gaussian_size, p.flat_scale)   # bkp:88-89
    sc[TIP_KEY] = tip_penalty_as_written(safe, p.chamfer_init_dist0)
    trad = (p.w_approach * sc["approach_score"] + p.w_sdf * sc["sdf_score"] + p.w_flat * sc["flatness_map"]
            + w_tip * (1 - sc[TIP_KEY]))
    trad = trad.astype(np.float32) * (1 - sc["stem_penalty"])                               # bkp:98-104
    valid = (sc["distance_map"] > p.min_edge_distance) & (safe > 0)                        # bkp:107
    trad = trad * valid
    sc["traditional_score"] = trad
    out = dict(safe=safe, scores=sc, valid=valid, theta=ref._last_angle, best_score=float(np.max(trad)))
    if np.any(trad > 0):                                                                    # bkp:111-117
        y, x = np.unravel_index(int(np.argmax(trad)), trad.shape)
        out.update(point=(int(x), int(y)), by_argmax=True)
    else:
        out.update(point=centroid(mask)[0], by_argmax=False)
    if out["point"] is None:
        out.update(point_3d=None, pre_grasp=None)
        return out
    g3 = ref.get_3d_grasp_point(out["point"], depth)
    out.update(point_3d=g3, pre_grasp=ref.calculate_pre_grasp_point(g3, safe))             # bkp:140-141: the eroded mask
    return out


def margin(trad):
    """Relative gap between the maximum of the float32 plane and the next smaller value (inf for a constant plane)."""
    v = np.unique(np.asarray(trad, np.float32))
    return math.inf if len(v) < 2 else float((v[-1] - v[-2]) / abs(v[-1]))


# ------------------------------------------------------------------------------------------------ inputs
def rotated_ellipse(H, W, cx, cy, a, b, ang):
    yy, xx = np.mgrid[0:H, 0:W]
    ca, sa = math.cos(ang), math.sin(ang)
    u = (xx - cx) * ca + (yy - cy) * sa
    v = -(xx - cx) * sa + (yy - cy) * ca
    return ((u / float(a)) ** 2 + (v / float(b)) ** 2 <= 1.0).astype(np.uint8)


def entry_scene(seed, sigma=0.003, H=240, W=320):
    """The whole-entry frames: one ellipse leaf with centre (165, 105), semi-axes 115 / 78, rotated by 0.3 * seed; depth a
    plane plus N(0, sigma) from default_rng(seed); the camera of O.synthetic_scene(240, 320, 3) with cx = 150, cy = 120."""
    mask = rotated_ellipse(H, W, 165, 105, 115, 78, 0.3 * seed)
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(seed)
    depth = (0.5 + 0.0004 * xx + 0.0002 * yy + rng.normal(0.0, sigma, (H, W))).astype(np.float32)
    P = np.array(O.synthetic_scene(240, 320, 3)[2], dtype=np.float64)
    P[0, 2], P[1, 2] = 150.0, 120.0
    return mask, depth, P


def largest_leaf(H, W, seed):
    """mask of the largest leaf of O.synthetic_scene(H, W, seed), the scene's depth and camera"""
    labels, depth, P = O.synthetic_scene(H, W, seed)
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    return (labels == ids[np.argmax(counts)]).astype(np.uint8), depth, P


def erosion_masks(H, W):
    """name -> u8 mask for the erosion tests: an ellipse, one running off the bottom-right corner, a one-pixel hole, a full
    frame (which must stay full: the border does not erode), an empty one"""
    out = {"ellipse": rotated_ellipse(H, W, W * 0.45, H * 0.5, W * 0.38, H * 0.4, 0.4),
           "corner": rotated_ellipse(H, W, W - 8, H - 6, W * 0.4, H * 0.45, -0.3),
           "full": np.ones((H, W), np.uint8), "empty": np.zeros((H, W), np.uint8)}
    m = out["ellipse"].copy()
    m[H // 2, min(W - 1, int(W * 0.45))] = 0
    out["hole"] = m
    return out
