"""Frames at the edges of what make_plan admits (8 <= H <= 16384, 8 <= W <= 8192, at most 8192 tiles of 64 x 16): plain data
shared by tests/test_frame_shapes_host.py (CPU: the premises, from the oracle alone) and tests/test_gpu_frame_shapes.py (the
HIP path against the oracle).  No device and no product import here.

A case is (H, W, mask kind, seed): the mask is made by `mask_of`, the depth is a ramp plus seeded noise, the camera's
principal point lies at a non-integer place inside the frame, and the constants are scaled to the frame's short side s
(`params_of`): the defaults' min_edge_distance = 20 leaves nothing valid on a frame 8 pixels high.  Values that are compared
with the fixed-point distance planes (min_edge_distance, optimal_distance) are small integers, exact in float32."""
import functools
from typing import NamedTuple

import numpy as np

INT_MAX = 2 ** 31 - 1

SMALL = [(8, 8), (8, 9), (9, 8), (8, 63), (8, 64), (8, 65), (15, 64), (16, 64), (17, 65), (16, 16), (31, 33), (33, 31),
         (12, 200), (200, 12)]
WIDE_TALL = [(24, 2112), (24, 4160), (24, 8192), (8, 8192), (16384, 8), (16384, 16)]
LARGE = (1009, 8129)    # 64 x 128 = exactly 8192 tiles, W > 4096: planes, validity and candidates only (the oracle needs seconds)
SHAPES = SMALL + WIDE_TALL + [LARGE]
# what make_plan refuses: H < 8, W < 8, W > 8192, H > 16384, and 9216 tiles
REFUSED_SHAPES = [(7, 64), (64, 7), (8, 8193), (16385, 8), (16384, 520)]

MASKS = ("full", "ellipse", "band", "ends", "corner", "last", "empty")
DEGENERATE = ("last", "empty")   # nothing valid by construction: a line one pixel wide has d_in = 1, the empty mask no pixel


def short_side(H, W):
    return min(H, W)


def params_of(H, W, top_k=4, **changes):
    """The full constant set (lg_params field names) for an H x W frame: the defaults scaled to the short side."""
    s = short_side(H, W)
    edge = 1 if s < 16 else 2
    out = dict(w_approach=0.4, w_sdf=0.3, w_flat=0.2, w_access=0.1, sdf_w_interior=0.4, sdf_w_align=0.4, sdf_w_sdf=0.2,
               optimal_distance=max(2, s // 5), access_w_dist=0.7, access_w_dir=0.3, flat_scale=5, iso_w_close=0.7, iso_w_wide=0.3,
               iso_ramp_top=1.0, iso_ramp_bottom=0.2, min_edge_distance=edge, stem_valid_thresh=0.8, stem_se=3, stem_bottom_div=3,
               top_k=top_k, nms_min_distance=edge, pregrasp_clearance=1, mask_is_bool=1, gaussian_size=3 if s < 16 else 5,
               chamfer_init_dist0=INT_MAX >> 2)
    unknown = set(changes) - set(out)
    assert not unknown, unknown
    out.update(changes)
    return out


def applicable(H, W, kind):
    """`ends` and `corner` need a long side: blobs of the short side's size with empty words between or beside them."""
    if kind in ("ends", "corner"):
        return max(H, W) >= 3 * min(H, W)
    return True


def mask_of(H, W, kind):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    if kind == "full":
        m[:] = 1
    elif kind == "ellipse":     # slanted (sheared), about 90 % of both sides
        u = (xx - (W - 1) / 2.0) / (0.45 * W)
        v = (yy - (H - 1) / 2.0) / (0.45 * H) - 0.3 * u
        m[u * u + v * v <= 1.0] = 1
    elif kind == "band":        # every column, not every row: runs as wide as the frame, zero pixels above and below
        m[max(1, H // 4):min(H - 1, H - H // 4), :] = 1
    elif kind == "ends":        # two blobs at the two ends of the long side, nothing between them
        s = min(H, W)
        r = 0.47 * s
        c = (s - 1) / 2.0
        for cx, cy in (((c, c), (W - 1 - c, H - 1 - c))):
            m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 1
    elif kind == "corner":      # one blob at the start of the long side: max d_out lies at the far frame corner, outside the window
        s = min(H, W)
        r, c = 0.47 * s, (s - 1) / 2.0
        m[(xx - c) ** 2 + (yy - c) ** 2 <= r * r] = 1
    elif kind == "last":        # tail bits of the last word, or the last tile row of one pixel
        if H % 16 == 1:
            m[H - 1, :] = 1
        else:
            m[:, W - 1] = 1
    else:
        assert kind == "empty", kind
    return m


@functools.lru_cache(maxsize=None)
def scene(H, W, kind, seed):
    """(mask uint8, depth float32, P): depth = ramp + seeded noise (as tests/golden/make_golden.py); the principal point at a
    non-integer place inside the frame."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (0.45 + 0.2 * xx / W + 0.1 * yy / H + rng.normal(0, 0.002, (H, W))).astype(np.float32)
    f = 1.2 * max(H, W)
    P = np.array([[f, 0, 0.37 * W + 0.305, -0.1 * f], [0, f, 0.61 * H + 0.205, 0], [0, 0, 1, 0]], np.float64)
    assert P[0, 2] != int(P[0, 2]) and P[1, 2] != int(P[1, 2]) and 0 < P[0, 2] < W - 1 and 0 < P[1, 2] < H - 1
    return mask_of(H, W, kind), depth, P


class Case(NamedTuple):
    H: int
    W: int
    kind: str
    seed: int = 0
    top_k: int = 4
    n_cand: int = 4        # candidates the oracle's walk hands out: top_k, or fewer where the frame runs out of free pixels

    @property
    def name(self):
        return f"{self.H}x{self.W}-{self.kind}"

    @property
    def shape(self):
        return (self.H, self.W)

    def params(self, **changes):
        return params_of(self.H, self.W, top_k=self.top_k, **changes)

    def scene(self):
        return scene(self.H, self.W, self.kind, self.seed)


# ----------------------------------------------------------------------------- what a shape is meant to reach (host arithmetic)
def words(W):
    return (W + 63) // 64


def tiles(H, W):
    return ((W + 63) // 64) * ((H + 15) // 16)


def sweep_geometry(W):
    """(threads, columns per thread) of the raster sweep's workgroup (lg_launch_dt)"""
    if W <= 2048:
        return (64 if W <= 256 else 128 if W <= 512 else 256 if W <= 1024 else 512), 4
    return (512 if W <= 4096 else 1024), 8


def norm5(dx, dy):
    """the closed-form norm of the 5 x 5 chamfer mask in 16.16 (lg_norm5)"""
    a, b = max(dx, dy), min(dx, dy)
    return (a - 2 * b) * 65536 + b * 143976 if 2 * b <= a else (a - b) * 143976 + (2 * b - a) * 91750


def far(H, W, init0=INT_MAX >> 2):
    """A distance in the frame can reach chamfer_init_dist0 (8192 px by default): OpenCV's border cells, which hold that value,
    then cap the transform, and the library sweeps the whole frame instead of a window or the row search (lg_dt_far)."""
    return norm5(W - 1, H - 1) >= init0


def window_fits(H, W):
    """a 32 x 32 CNN window lies inside the frame somewhere (x - 16 >= 0, x + 16 <= W)"""
    return H >= 32 and W >= 32


def reach(H, W):
    """the paths an H x W frame takes, as a set of tags"""
    r = set()
    if H < 16 or W < 16:
        r.add("form1_forced")
    if H == 16 or W == 16:
        r.add("sixteen")
    if 2048 < W <= 4096:
        r.add("W_2049_4096")
    if 4096 < W < 8192:
        r.add("W_4097_8191")
    if W == 8192:
        r.add("W_8192")
    if H == 16384:
        r.add("H_16384")
    if tiles(H, W) == 8192:
        r.add("tiles_8192")
    if tiles(H, W) == 1:
        r.add("one_tile")
    if words(W) == 1 and W % 64:
        r.add("one_word_tail")
    if H < 32 and W < 32:
        r.add("window_over_all_borders")
    if words(W) > 64:
        r.add("hrun_pieces")
    if W > 2048:
        r.add("iso_sweep_32")
    return r


# ----------------------------------------------------------------------------- the tables
# The whole selection is compared with the ORACLE's own (its planes, its walk, its pick) on these: one per shape, the seed
# chosen with the oracle alone so that no pick of the walk and no two pick scores lie nearer than 1e-3 relative without being
# the same float, with a bool and with a uint8 mask (tests/test_frame_shapes_host.py asserts it).  Each seed is the first of
# 0 .. 39 that does.  (1009, 8129) is not here: planes, validity and candidates only.
END_TO_END = [
    Case(8, 8, "ellipse", 0), Case(8, 9, "ellipse", 1), Case(9, 8, "ellipse", 0), Case(8, 63, "ellipse", 2),
    Case(8, 64, "ellipse", 0), Case(8, 65, "ellipse", 0), Case(15, 64, "ellipse", 0), Case(16, 64, "ellipse", 0),
    Case(17, 65, "ellipse", 2), Case(16, 16, "ellipse", 0), Case(31, 33, "ellipse", 0), Case(33, 31, "ellipse", 11),
    Case(12, 200, "ellipse", 2), Case(200, 12, "ellipse", 0), Case(24, 2112, "ellipse", 21), Case(24, 4160, "ellipse", 1),
    Case(24, 8192, "ellipse", 2), Case(8, 8192, "ellipse", 0), Case(16384, 8, "ellipse", 1), Case(16384, 16, "ellipse", 1),
]
E2E_BY_SHAPE = {c.shape: c for c in END_TO_END}

# a top_k the frame cannot fill: the walk suppresses (4 d + 1)^2 pixels per pick (d = nms_min_distance) and hands out invalid
# pixels before it stops, so the count is a matter of geometry; the numbers are the oracle's
RUN_OUT = [Case(8, 8, "ellipse", 0, top_k=20, n_cand=8), Case(8, 9, "full", 0, top_k=20, n_cand=9),
           Case(9, 8, "band", 0, top_k=64, n_cand=9), Case(8, 63, "ellipse", 0, top_k=64, n_cand=62)]


def plane_cases(shape):
    """every applicable mask of one shape, top_k = 4 (the large frame: the ellipse alone)"""
    H, W = shape
    if shape == LARGE:
        return [Case(H, W, "ellipse", 0)]
    e = E2E_BY_SHAPE[shape]
    out = []
    for k in MASKS:
        if applicable(H, W, k):
            out.append(e if k == e.kind else Case(H, W, k, 0))
    return out


# ----------------------------------------------------------------------------- the oracle on a case
@functools.lru_cache(maxsize=None)
def run(case, with_cnn=False, mask_is_bool=1):
    """What tests/param_oracle.run gives for a named scene, for a Case: the oracle's select_grasp_point(return_debug=True) under
    the case's constants plus every candidate's pre-grasp point."""
    from tests import param_oracle as PO

    mask, depth, P = case.scene()
    ref = PO.oracle(P, case.params(mask_is_bool=mask_is_bool), with_cnn)
    with np.errstate(all="ignore"):
        triple, dbg = ref.select_grasp_point(mask, depth, return_debug=True)
        pre = [ref.calculate_pre_grasp_point(ref.get_3d_grasp_point(c, depth), mask) for c in dbg["candidates"]]
    return dict(triple=triple, scores=dbg["scores"], valid=dbg["valid"], candidates=dbg["candidates"],
                ml_scores=dbg["ml_scores"], pregrasp=pre, ref=ref)
