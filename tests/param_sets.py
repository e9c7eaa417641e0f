"""Named sets of lg_params constants away from the reference's values: plain data shared by tests/test_oracle_params.py (CPU:
the oracle alone shows that every set moves the output it feeds on its scene) and tests/test_gpu_params.py (the HIP path
against the oracle under the same set).  A set is "the defaults with these fields changed", paired with one seeded scene.

Values compared with integers or with the fixed-point distance planes (min_edge_distance, optimal_distance, the
thresholds) are exactly representable in float32; every weight stays within [-1, 1], so every plane keeps the magnitude the
project's tolerance (rtol 1e-4, atol 1e-6) was set for."""
from typing import NamedTuple, Optional

INT_MAX = 2 ** 31 - 1

# lg_default_params (include/leafgrasp.h), without the camera
DEFAULTS = dict(
    w_approach=0.4, w_sdf=0.3, w_flat=0.2, w_access=0.1, sdf_w_interior=0.4, sdf_w_align=0.4, sdf_w_sdf=0.2,
    optimal_distance=20, access_w_dist=0.7, access_w_dir=0.3, flat_scale=5, iso_w_close=0.7, iso_w_wide=0.3,
    iso_ramp_top=1.0, iso_ramp_bottom=0.2, min_edge_distance=20, stem_valid_thresh=0.8, stem_se=30, stem_bottom_div=3,
    top_k=20, nms_min_distance=10, pregrasp_clearance=15, mask_is_bool=1, gaussian_size=5, chamfer_init_dist0=INT_MAX >> 2)

FLOAT_FIELDS = ("w_approach", "w_sdf", "w_flat", "w_access", "sdf_w_interior", "sdf_w_align", "sdf_w_sdf", "optimal_distance",
                "access_w_dist", "access_w_dir", "flat_scale", "iso_w_close", "iso_w_wide", "iso_ramp_top", "iso_ramp_bottom",
                "min_edge_distance", "stem_valid_thresh")
# the fields no test moved before this table existed
NEVER_TESTED = FLOAT_FIELDS + ("stem_se", "stem_bottom_div", "pregrasp_clearance")

# (H, W, seed, leaf id[, cx / W]) of oracle.synthetic_scene; a fifth entry moves the camera's principal point sideways (the
# pre-grasp walk of calculate_pre_grasp_point only leaves the leaf for a grasp far off the optical axis: it accepts a point
# once it lies 0.05 m from the grasp ACROSS the axis).  Counts at the defaults, from the oracle:
SCENES = {
    "cut": (200, 1028, 4, 1),     # 26397 px leaf cut by the stem band: 9261 stem, 11139 valid; W % 4 == 0, W % 64 != 0
    "cut2": (200, 1028, 1, 1),    # 27094 px, 8380 stem, 11689 valid
    "band": (301, 517, 2, 1),     # 5941 px, 3263 stem, 640 valid; odd W
    "rim": (301, 517, 4, 5),      # 6045 px leaf touching the frame border, 369 stem, 1594 valid
    "wide_rim": (200, 1028, 3, 5),  # 25159 px on the frame border, 3509 stem, 15999 valid
    "mid": (270, 360, 4, 1),      # 3243 px mid-frame (85 px from every border), no stem at the defaults, 418 valid
    "top": (301, 517, 1, 1),      # 6855 px, no stem, 1526 valid
    # pre-grasp frames: (a) the pick mid-frame (122 px from every border), camera far to the left: clearances 0, 1, 4, 30, 31
    # each give another pre-grasp point than 15
    "offaxis": (270, 360, 1, 1, -1.5),
    # (b) a hand-made 36 x 200 strip along the top border (rows 0..35, columns 100..299) over the depth of seed 4, camera to the
    # right, min_edge_distance 5.5: the pick (281, 5) lies 5 px from the frame (30 / 31 move its pre-grasp point), the second
    # candidate (259, 14) 14 px from it (0, 1, 30, 31 all move it)
    "top_strip": (301, 517, 4, "strip", 1.8),
    # full size: a 104222 px leaf cut by the stem band under the defaults (65304 stem) and under both all-different sets
    # (36644 and 23512 stem)
    "full": (1080, 1920, 31, 4),
}

# the output a field feeds (what must move when the field moves)
FEEDS = dict(
    w_approach="traditional_score", w_sdf="traditional_score", w_flat="traditional_score", w_access="traditional_score",
    sdf_w_interior="sdf_score", sdf_w_align="sdf_score", sdf_w_sdf="sdf_score", optimal_distance="sdf_score",
    access_w_dist="accessibility_map", access_w_dir="accessibility_map", flat_scale="flatness_map",
    iso_w_close="isolation_map", iso_w_wide="isolation_map", iso_ramp_top="isolation_map", iso_ramp_bottom="isolation_map",
    min_edge_distance="valid", stem_valid_thresh="valid", stem_se="stem_penalty", stem_bottom_div="stem_penalty",
    pregrasp_clearance="pregrasp", gaussian_size="flatness_map", chamfer_init_dist0="isolation_map", top_k="candidates",
    nms_min_distance="candidates")


class ParamSet(NamedTuple):
    name: str
    changes: dict
    scene: str = "cut"
    mask_dtype: str = "bool"          # "uint8": the mirror derives mask_is_bool = 0, border candidates are scored
    feeds: Optional[tuple] = None     # outputs that must move on the scene; None = FEEDS of every changed field
    versus: Optional[dict] = None     # the set to differ from, when it is not the defaults (see thresh_1)
    ties: bool = False                # meant to tie: exact zeros / equal floats, decided by (score desc, flat index desc)

    def outputs(self):
        if self.feeds is not None:
            return self.feeds
        return tuple(dict.fromkeys(FEEDS[k] for k in self.changes if k in FEEDS))


def _one(field, value, scene="cut", **kw):
    return ParamSet(f"{field}={value}", {field: value}, scene, **kw)


ONE_AT_A_TIME = [
    _one("w_approach", 0.25), _one("w_sdf", 0.55), _one("w_flat", 0.45), _one("w_access", 0.35),
    _one("sdf_w_interior", 0.15), _one("sdf_w_align", 0.65), _one("sdf_w_sdf", 0.45),
    _one("optimal_distance", 3), _one("optimal_distance", 47.5, "cut2"),
    _one("access_w_dist", 0.45), _one("access_w_dir", 0.55), _one("flat_scale", 2.5),
    _one("iso_w_close", 0.35), _one("iso_w_wide", 0.6), _one("iso_ramp_top", 0.5), _one("iso_ramp_bottom", 0.75),
    _one("min_edge_distance", 7.5, "band"), _one("min_edge_distance", 33.25, "cut2"),
    _one("stem_valid_thresh", 1.5), _one("stem_se", 47, "band"), _one("stem_bottom_div", 5),
    _one("pregrasp_clearance", 4, "offaxis"),
]

EDGES = [
    _one("stem_se", 1), _one("stem_se", 2, "band"), _one("stem_se", 31, "cut2"),
    # ellipse 29 and ellipse 30 both reach 14 rows up from the band (the 30th row of ellipse 30 points down, into the band), so
    # their stem planes differ at the two ends of the frontier only (12 .. 19 px on every surveyed frame); the neighbour that 29
    # must be told apart from is 31, which reaches 15 rows up (tests/test_oracle_params.py holds every span of 1..64 exactly)
    ParamSet("stem_se=29", {"stem_se": 29}, "cut2", versus={"stem_se": 31}),
    _one("stem_se", 63, "band"), _one("stem_se", 64),
    _one("stem_bottom_div", 1, "mid"), _one("stem_bottom_div", 2, "top"), _one("stem_bottom_div", 7),
    # larger than H = 301: the reference's bottom[-0:, :] = 1 marks the whole frame, every leaf pixel is stem
    _one("stem_bottom_div", 500, "top"),
    *[_one("pregrasp_clearance", c, "offaxis") for c in (0, 1, 30, 31)],
    *[ParamSet(f"pregrasp_clearance={c}_at_the_border", {"pregrasp_clearance": c, "min_edge_distance": 5.5}, "top_strip",
               feeds=("pregrasp",), versus={"min_edge_distance": 5.5}) for c in (0, 1, 30, 31)],
    _one("stem_valid_thresh", 0),      # stem is 0 / 1: nothing is below 0, no pixel valid
    # stem < 1.0 is what stem < 0.8 is for a 0 / 1 plane: this set equals the defaults BY DESIGN and guards the strictness of the
    # comparison (a `<=` would admit every stem pixel); what it must differ from is the other side, 1.5
    ParamSet("stem_valid_thresh=1.0", {"stem_valid_thresh": 1.0}, "cut", versus={"stem_valid_thresh": 1.5}),
    _one("flat_scale", 0), _one("flat_scale", 50),
    ParamSet("ramp_rising", {"iso_ramp_top": 0.25, "iso_ramp_bottom": 0.875}, "band"),
    ParamSet("uint8_rim", {"min_edge_distance": 0, "w_sdf": 0.2, "w_access": 0.3}, "rim", mask_dtype="uint8"),
    _one("min_edge_distance", 0, "wide_rim"),
]

SIGNS = [
    _one("w_access", 0), _one("w_flat", 0),
    # approach is ~1 on the leaf: every valid pixel scores below the +0.0 of the invalid ones
    ParamSet("negative_approach", {"w_approach": -0.9}, "cut2"),
    # mildly negative: the leaf's scores straddle zero
    ParamSet("negative_mixed", {"w_approach": -0.25, "w_sdf": 0.5}, "band"),
    _one("sdf_w_sdf", -0.5), _one("sdf_w_interior", -0.3, "cut2"),
]

_ALL_A = dict(w_approach=0.31, w_sdf=0.27, w_flat=0.23, w_access=0.19, sdf_w_interior=0.45, sdf_w_align=0.35,
              sdf_w_sdf=0.15, optimal_distance=14.5, access_w_dist=0.6, access_w_dir=0.25, flat_scale=3.5, iso_w_close=0.55,
              iso_w_wide=0.5, iso_ramp_top=0.9, iso_ramp_bottom=0.125, min_edge_distance=12.25, stem_valid_thresh=0.625,
              stem_se=23, stem_bottom_div=4, top_k=12, nms_min_distance=7, pregrasp_clearance=9, gaussian_size=3)
_ALL_B = dict(w_approach=0.12, w_sdf=0.46, w_flat=0.33, w_access=0.08, sdf_w_interior=0.22, sdf_w_align=0.52,
              sdf_w_sdf=0.28, optimal_distance=26.5, access_w_dist=0.82, access_w_dir=0.17, flat_scale=7.25, iso_w_close=0.38,
              iso_w_wide=0.62, iso_ramp_top=0.75, iso_ramp_bottom=0.4375, min_edge_distance=16.5, stem_valid_thresh=0.9375,
              stem_se=41, stem_bottom_div=5, top_k=33, nms_min_distance=14, pregrasp_clearance=21, gaussian_size=7,
              chamfer_init_dist0=INT_MAX)
_ALL_FEEDS = ("traditional_score", "sdf_score", "accessibility_map", "flatness_map", "isolation_map", "valid", "stem_penalty",
              "candidates")
ALL_DIFFERENT = [ParamSet("all_different_a", _ALL_A, "cut", feeds=_ALL_FEEDS),
                 ParamSet("all_different_b", _ALL_B, "cut2", feeds=_ALL_FEEDS),
                 ParamSet("all_different_a_1080p", _ALL_A, "full", feeds=_ALL_FEEDS),
                 ParamSet("all_different_b_1080p", _ALL_B, "full", feeds=_ALL_FEEDS)]

# a steep term for the sets whose whole selection is held to the oracle's (END_TO_END): exp(-50 |grad|) of the depth's noise
# separates neighbouring pixels' scores by per cent, where the smooth terms alone leave 1e-4 between a pick and its neighbour
_STEEP = {"w_flat": 1.0, "flat_scale": 50}
COMBINED = [
    ParamSet("gauss1_top1", {"gaussian_size": 1, "top_k": 1, **_STEEP}, "cut2"),
    ParamSet("gauss7_top2_nms0", {"gaussian_size": 7, "top_k": 2, "nms_min_distance": 0, "stem_se": 17, **_STEEP}, "cut2"),
    ParamSet("intmax_top64_nms25", {"chamfer_init_dist0": INT_MAX, "top_k": 64, "nms_min_distance": 25, "iso_w_close": 0.2,
                                    "min_edge_distance": 5.5}, "cut2"),
    ParamSet("nms0_edge0", {"nms_min_distance": 0, "min_edge_distance": 0, "optimal_distance": 9}, "wide_rim"),
    ParamSet("edge0_top3_uint8", {"min_edge_distance": 0, "top_k": 3, "nms_min_distance": 40, "w_approach": 0.3, **_STEEP},
             "cut2", mask_dtype="uint8"),
    ParamSet("negative_mixed_top3", {"w_approach": -0.25, "w_sdf": 0.5, "top_k": 3, "nms_min_distance": 30, **_STEEP}, "mid"),
    ParamSet("all_different_a_top4", dict(_ALL_A, top_k=4, nms_min_distance=45, **_STEEP), "rim", feeds=_ALL_FEEDS),
    # the sets meant to tie, on 17 valid pixels (min_edge_distance just under the leaf's largest d_in of 28.4): one pick on the
    # leaf, then nineteen exact ties -- w_flat = 0 makes every constant tile score exactly 0 like an invalid pixel; with
    # flat_scale = 0 the flatness is exactly 1 everywhere -- which only the total order (score desc, flat index desc) decides
    ParamSet("w_flat=0_few_valid", {"w_flat": 0, "min_edge_distance": 27.5}, "mid", ties=True),
    ParamSet("flat_scale=0_few_valid", {"flat_scale": 0, "min_edge_distance": 27.5}, "mid", ties=True),
]

SETS = ONE_AT_A_TIME + EDGES + SIGNS + ALL_DIFFERENT + COMBINED
BY_NAME = {s.name: s for s in SETS}
assert len(BY_NAME) == len(SETS)

# The sets whose candidate list and pick are compared with the ORACLE's own (its planes, not the device's).  Fair only where
# no plane error within the tolerance can change a pick: tests/test_oracle_params.py asserts, from the oracle alone, that at
# every pick of the greedy walk the picked pixel and the best pixel the walk could have taken instead (its neighbours
# included) are 1e-3 relative apart or exactly equal, and the same for the deciding pick scores.  Every other set's candidates
# are held bit-exact to the oracle's walk over the device's own planes instead.
END_TO_END = ("gauss1_top1", "gauss7_top2_nms0", "edge0_top3_uint8", "negative_approach", "negative_mixed_top3",
              "w_flat=0_few_valid", "flat_scale=0_few_valid", "all_different_a_top4")
# the sets whose sparse (no plane output) and dense calls must give the same rows: the constant-tile value w_flat *
# flatness(flat_scale), the validity thresholds and negative scores
SPARSE_DENSE = ("w_flat=0.45", "w_flat=0", "flat_scale=2.5", "flat_scale=0", "flat_scale=50", "stem_valid_thresh=0",
                "stem_valid_thresh=1.0", "stem_valid_thresh=1.5", "min_edge_distance=0", "min_edge_distance=7.5",
                "min_edge_distance=33.25", "negative_approach", "negative_mixed", "all_different_a", "all_different_b")

# what make_plan refuses (LG_ERR_INVALID): field, value
REFUSED = [("stem_se", 0), ("stem_se", 65), ("stem_bottom_div", 0), ("pregrasp_clearance", -1), ("pregrasp_clearance", 32),
           ("nms_min_distance", -1), ("top_k", 0), ("top_k", 65)]


def params_of(changes=None):
    """The full constant set (lg_params field names) of a ParamSet, a name or a dict of changes: the defaults with them applied."""
    if isinstance(changes, str):
        changes = BY_NAME[changes]
    out = dict(DEFAULTS)
    if isinstance(changes, ParamSet):
        out["mask_is_bool"] = 1 if changes.mask_dtype == "bool" else 0
        changes = changes.changes
    unknown = set(changes or ()) - set(out)
    assert not unknown, unknown
    out.update(changes or {})
    return out
