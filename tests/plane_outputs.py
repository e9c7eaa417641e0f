"""Cases for the plane kernel under every subset of outputs include/leafgrasp.h allows (out_maps[i] "may be NULL = not wanted",
out_valid "may be NULL"): plain data shared by tests/test_plane_outputs_host.py (CPU: the premises, from the oracle and host
arithmetic) and tests/test_gpu_plane_outputs.py (the HIP path against the oracle).  No device and no product import here.

Two frames, 104 x 264 (W % 4 == 0: the vector stores) and 104 x 263 (the scalar stores).  Tiles are 64 x 16: 5 x 7 of them, a
last tile column 8 / 7 pixels wide, a last tile row 8 rows high.  The smallest frame that has at once an interior tile column on
the 16-byte staging path (tx0 >= 4 and tx0 + 68 <= W: tile columns 1 to 3), tiles on the constant path, tiles outside the
sweep window (where the plane kernel itself writes distance = 0) and a partial last tile row and column.

Scenes (depth and P: tests/frame_shapes.scene of the seed):
  interior   a slanted ellipse, u = (x - 139.5) / 68, v = (y - 52) / 27 - 0.25 u, u^2 + v^2 <= 1: x 72..207, y 25..79.  Tile
             columns 0 and 4 and tile rows 0 and 6 are far from it at every smoothing radius (reach <= 4 px).
  corner     the same ellipse about (30, 12), running off the top-left corner, and a disc of radius 13 about (W - 8, 66) that
             touches the right edge: reflect staging and the partial last column on the stencil path.
Constants: frame_shapes.params_of(top_k = 4, min_edge_distance = 6, nms_min_distance = 6, stem_se = 9, optimal_distance = 10,
pregrasp_clearance = 5, gaussian_size = g) plus param_sets._STEEP (w_flat = 1, flat_scale = 50): the flatness term decides the
picks, and flatness is the term whose rounding differs between the forms of the kernel.
One seed per (width, gaussian_size): the first of 0 .. 39 for which the oracle's selection on `interior` has no near-tie
(tests/test_plane_outputs_host.py asserts both the bound and that every earlier seed misses it)."""
import functools
import itertools

import numpy as np

from tests import frame_shapes as FS
from tests import param_sets as PS

H = 104
WIDTHS = (264, 263)
SIZES = (1, 3, 5, 7)
SCENES = ("interior", "corner")
TOP_K = 4
TW, TH = 64, 16

# lg_map indices (include/leafgrasp.h); PLANES[i] is the oracle's key of out_maps[i]
SDF, APPROACH, FLATNESS, ISOLATION, DISTANCE, ACCESS, STEM, TRADITIONAL = range(8)
PLANES = ("sdf_score", "approach_score", "flatness_map", "isolation_map", "distance_map", "accessibility_map", "stem_penalty",
          "traditional_score")
EXACT = (DISTANCE, STEM)       # bit for bit; the other six: rtol 1e-4 / atol 1e-6
ALL = frozenset(range(8))

SEEDS = {(264, 1): 0, (264, 3): 2, (264, 5): 1, (264, 7): 0, (263, 1): 1, (263, 3): 1, (263, 5): 1, (263, 7): 0}


def params_of(W, g, **changes):
    return FS.params_of(H, W, top_k=TOP_K, **{**dict(min_edge_distance=6, nms_min_distance=6, stem_se=9, optimal_distance=10,
                                                     pregrasp_clearance=5, gaussian_size=g, **PS._STEEP), **changes})


def _ellipse(W, cx, cy):
    yy, xx = np.mgrid[0:H, 0:W]
    u = (xx - cx) / 68.0
    v = (yy - cy) / 27.0 - 0.25 * u
    return u * u + v * v <= 1.0


@functools.lru_cache(maxsize=None)
def mask_of(W, scene):
    if scene == "interior":
        return _ellipse(W, 139.5, 52.0).astype(np.uint8)
    assert scene == "corner", scene
    yy, xx = np.mgrid[0:H, 0:W]
    return (_ellipse(W, 30.0, 12.0) | ((xx - (W - 8)) ** 2 + (yy - 66) ** 2 <= 13 ** 2)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(W, name, seed):
    """(mask uint8, depth float32, P)"""
    _, depth, P = FS.scene(H, W, "empty", seed)
    return mask_of(W, name), depth, P


@functools.lru_cache(maxsize=None)
def run(W, name, g, seed=None, with_cnn=False, default_params=False):
    """The oracle on a case: what tests/frame_shapes.run gives, plus theta.  default_params: under lg_default_params (what a
    call with p = NULL computes: the reference's constants, camera 707 / 494 / f unset = 0)."""
    from oracle import lg_oracle as O
    from tests import param_oracle as PO

    seed = SEEDS[(W, g)] if seed is None else seed
    mask, depth, P = scene(W, name, seed)
    if default_params:
        assert g == 5 and not with_cnn
        ref = O.RefGraspPointSelector(params=PS.params_of({}))
        ref.camera_cx, ref.camera_cy, ref.f_norm = 707.0, 494.0, 0.0   # (set_camera_params would divide by f)
    else:
        ref = PO.oracle(P, params_of(W, g), with_cnn)
    with np.errstate(all="ignore"):
        if default_params:   # the planes alone: f = 0 gives no 3-D point
            sc = ref._calculate_all_scores(mask, depth)
            return dict(scores=sc, valid=ref._get_valid_regions(mask, sc), theta=ref._last_angle, ref=ref)
        triple, dbg = ref.select_grasp_point(mask, depth, return_debug=True)
        pre = [ref.calculate_pre_grasp_point(ref.get_3d_grasp_point(c, depth), mask) for c in dbg["candidates"]]
    assert isinstance(O.INIT_DIST0, int)
    return dict(triple=triple, scores=dbg["scores"], valid=dbg["valid"], candidates=dbg["candidates"], ml_scores=dbg["ml_scores"],
                pregrasp=pre, theta=ref._last_angle, ref=ref)


# ----------------------------------------------------------------------------- subsets: (frozenset of plane indices, validity given)
EXHAUSTIVE = [(frozenset(i for i in range(8) if bits >> i & 1), bool(v)) for bits in range(256) for v in (0, 1)]

NAMED = ([("validity alone", frozenset(), True), ("all planes, no validity", ALL, False)]
         + [(f"{PLANES[i]} alone", frozenset([i]), True) for i in range(8)]
         + [(f"all but {PLANES[i]}", ALL - {i}, True) for i in range(8)]
         + [("distance and traditional alone", frozenset([DISTANCE, TRADITIONAL]), False),
            ("all but distance and traditional", ALL - {DISTANCE, TRADITIONAL}, True)])
FULL = (ALL, True)
NOTHING = (frozenset(), False)


def subset_id(planes, valid):
    return "".join(str(i) for i in sorted(planes)) + ("v" if valid else "") or "none"


def store_form(planes, valid, entry="score_maps", model=False):
    """Which store form of lg_final_kernel a call reaches -- a pure function of the pointers, the entry and the model
    (lg_select.hip: take_planes, lg_planes.hip: lg_launch_final).  take_planes fills in workspace planes for distance and
    traditional always, for all eight when a model is loaded and the planes are not deferred, and the workspace validity plane
    when out_valid is NULL; lg_launch_final then takes ALL when no pointer is left NULL.
      "all"      every plane given (with or without validity), or a non-sparse lg_select_grasp* call with a model loaded
      "score"    lg_select_grasp* with no plane and no validity (sparse mode, deferred planes)
      "partial"  everything else: lg_final_kernel<VEC, false, R>"""
    if entry != "score_maps" and not planes and not valid:
        return "score"
    if planes | {DISTANCE, TRADITIONAL} == ALL or (entry != "score_maps" and model):
        return "all"
    return "partial"


def instantiation(W, g, planes, valid, entry="score_maps", model=False):
    """(VEC, ALL, R, SCORE) of lg_final_kernel<VEC, ALL, R, SCORE>"""
    f = store_form(planes, valid, entry, model)
    return (W % 4 == 0, f == "all", g // 2, f == "score")


PARTIAL_FORMS = [(vec, False, r, False) for vec in (True, False) for r in (0, 1, 2, 3)]


# ----------------------------------------------------------------------------- tile classes (host arithmetic)
def tile_grid(W):
    return (W + TW - 1) // TW, (H + TH - 1) // TH


def tile_classes(W, name, g, window):
    """Counts per case.  `window`: (wx0, wx1, wy0, wy1) of the frame's sweep window (lg_window_from_box).
      far       tiles whose look at the mask cannot meet its bounding box (constant without a bit-row test)
      near      the others (tests/near_tiles_ref.near_map, halo = g / 2 + 1)
      stencil   near tiles whose bit-row test finds a mask bit (near_tiles_ref.reach_map): the full path
      constant  far tiles + near tiles whose test finds nothing
      outside   tiles whose origin lies outside the sweep window: the plane kernel writes distance = 0 there
      staged16  stencil tiles with tx0 >= 4 and tx0 + 68 <= W: the 16-byte staging loads (only where W % 4 == 0)
    plus the near / stencil maps themselves."""
    from tests import near_tiles_ref as NT

    mask = mask_of(W, name)
    halo = g // 2 + 1
    near = NT.near_map(NT.bbox(mask), H, W, halo)
    stencil = NT.reach_map(mask, halo)
    assert not (stencil & ~near).any()
    tiles_x, tiles_y = tile_grid(W)
    wx0, wx1, wy0, wy1 = window
    outside = np.zeros_like(near)
    wide = np.zeros_like(near)
    for ty, tx in itertools.product(range(tiles_y), range(tiles_x)):
        tx0, ty0 = tx * TW, ty * TH
        outside[ty, tx] = not (wx0 <= tx0 < min(W, wx1) and wy0 <= ty0 < wy1)
        wide[ty, tx] = tx0 >= 4 and tx0 + TW + 4 <= W
    return dict(far=int((~near).sum()), near=int(near.sum()), stencil=int(stencil.sum()), constant=int((~stencil).sum()),
                outside=int(outside.sum()), staged16=int((stencil & wide).sum()), near_map=near, stencil_map=stencil,
                outside_map=outside)
