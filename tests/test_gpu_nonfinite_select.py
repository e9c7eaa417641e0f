"""Depth holes through the whole selection with a model loaded, against the oracle.

ON the leaf a hole follows the reference everywhere: NaN planes over its 7 x 7 reach, NaN candidates first, and -- the part
only a loaded model shows -- a NaN logit for every candidate whose 32 x 32 window holds a non-finite value (torch's relu and
max_pool2d propagate it), hence NaN `ml_score`, `ml_confidence` and `combined` in its row, and such a candidate is never
taken by ML.  OFF the leaf the planes ignore the hole (the documented deviation) but the depth channel of a patch still reads
it: the candidate list and every traditional score are those of the cleaned frame, and a candidate with the hole in its
window has a NaN ML score all the same.

Two small frames with an ellipse for a leaf (the depth of O.synthetic_scene); holes sit `off` pixels from clean candidates,
toward the leaf's middle row.  Every case asserts from the oracle alone, before the device runs, that at least 2 candidates
have a finite traditional score and a NaN ml, and at least 2 scored candidates a finite ml."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests.test_gpu_grasp_candidates import (_assert_order_is_the_rule, _assert_rank0_is_the_result,  # noqa: E402
                                             _assert_rows_match_oracle, _by_index, _oracle_rows, _params, _valid_rows)

# name: (H, W, ellipse centre x, y, semi-axes x, y, the clean candidates that get a hole)
FRAMES = {"A": (400, 520, 260, 200, 150, 90, (1, 3, 5, 8)), "B": (160, 224, 112, 80, 80, 50, (1, 3, 5))}
# hole value -> pixels between the clean candidate and its hole, per frame.  12 is the placement for NaN; with an infinity
# there the clean candidates next to the holes are all suppressed by the NaN candidates that lead the list and fewer than 2
# candidates keep a finite traditional score beside a NaN ml, so the infinite holes sit further in.
OFFSETS = {"nan": {"A": 12, "B": 12}, "zero": {"A": 12, "B": 12}, "+inf": {"A": 18, "B": 22}, "-inf": {"A": 18, "B": 22}}
VALUES = {"nan": np.float32(np.nan), "zero": np.float32(0.0), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}


def _ellipse(H, W, cx, cy, a, b):
    yy, xx = np.mgrid[:H, :W]
    return ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0


@functools.lru_cache(maxsize=None)
def _clean(name):
    """(mask bool, depth, P, the oracle's candidates of the clean frame)."""
    H, W, cx, cy, a, b, _ = FRAMES[name]
    _, depth, P = O.synthetic_scene(H, W, 5)
    mask = _ellipse(H, W, cx, cy, a, b)
    ref = O.RefGraspPointSelector(cnn=None)
    ref.set_camera_params(P)
    _, dbg = ref.select_grasp_point(mask.astype(np.uint8), depth, mask_is_bool=True, return_debug=True)
    return mask, depth, P, dbg["candidates"]


@functools.lru_cache(maxsize=None)
def _frame(name, value):
    """(mask, clean depth, holed depth, P, hole pixels (x, y)): one hole per chosen clean candidate, OFFSETS px toward the
    leaf's middle row."""
    mask, depth, P, cands = _clean(name)
    cy, which = FRAMES[name][3], FRAMES[name][6]
    d = depth.copy()
    holes = []
    for i in which:
        x, y = cands[i]
        hy = y + OFFSETS[value][name] * int(np.sign(cy - y))
        assert mask[hy, x]
        d[hy, x] = VALUES[value]
        holes.append((x, hy))
    return mask, depth, d, P, holes


def frame_b():
    """Frame B with NaN holes (for tests/test_gpu_cnn_nonfinite.py: the staged patches)."""
    return _frame("B", "nan")


def _classes(orows):
    """(NaN traditional, finite traditional and NaN ml, finite ml, unscored) candidate indices of oracle rows."""
    nan_t = [i for i, o in enumerate(orows) if math.isnan(o["trad"])]
    nan_ml = [i for i, o in enumerate(orows) if not math.isnan(o["trad"]) and o["ml"] is not None and math.isnan(o["ml"])]
    fin_ml = [i for i, o in enumerate(orows) if o["ml"] is not None and not math.isnan(o["ml"])]
    return nan_t, nan_ml, fin_ml, [i for i, o in enumerate(orows) if o["ml"] is None]


@functools.lru_cache(maxsize=None)
def _expected(name, value):
    """The oracle's triple and rows of the holed frame, after the oracle-only precondition."""
    mask, _, holed, P, _ = _frame(name, value)
    exp, orows = _oracle_rows(P, mask, holed, True, mask_is_bool=True)
    nan_t, nan_ml, fin_ml, unscored = _classes(orows)
    if value == "zero":       # the finite control: nothing is NaN
        assert not nan_t and not nan_ml and len(fin_ml) >= 2, (name, value)
    else:
        assert len(nan_ml) >= 2 and len(fin_ml) >= 2, (name, value, nan_t, nan_ml, fin_ml, unscored)
    return exp, orows


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_triple(got, exp):
    assert tuple(got[0]) == tuple(exp[0]), (got, exp)
    np.testing.assert_allclose(np.array(got[1], np.float64), np.array(exp[1], np.float64), rtol=1e-5, equal_nan=True)
    assert (got[2] is None) == (exp[2] is None), (got, exp)
    if exp[2] is not None:
        np.testing.assert_allclose(np.array(got[2], np.float64), np.array(exp[2], np.float64), rtol=1e-5, equal_nan=True)


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


HANDLES = ("default", "LG_CNN_PRUNE=0", "LG_DEFER_PLANES=0")


@pytest.fixture(scope="module")
def handles(L):
    """name -> selector with the standard model: a default handle and one created under each switch (read at lg_create)."""
    mp = pytest.MonkeyPatch()
    out = {}
    for name in HANDLES:
        for k in ("LG_CNN_PRUNE", "LG_DEFER_PLANES"):
            mp.delenv(k, raising=False)
        if name != "default":
            k, v = name.split("=")
            mp.setenv(k, v)
        s = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
        s.set_cnn_state_dict(_params())
        out[name] = s
    mp.undo()
    yield out
    for s in out.values():
        s.clear_cnn()


CASES = [(f, v) for f in FRAMES for v in ("nan", "+inf", "-inf", "zero")]


@pytest.mark.parametrize("name,value", CASES, ids=[f"{f}{v}" for f, v in CASES])
def test_holes_on_the_leaf(L, handles, name, value):
    exp, orows = _expected(name, value)          # (oracle only: asserts the precondition before any device call)
    mask, _, holed, P, _ = _frame(name, value)
    m, d = _dev(mask[None]), _dev(holed[None])
    raw = {}
    for hname, s in handles.items():
        s.set_camera_params(P)
        triples, cands = s.select_grasp_candidates_batch(m, d)
        res_c = bytes(s.last_results)
        rows = _valid_rows(cands[0])
        what = f"frame {name} {value}, {hname}"
        _assert_rows_match_oracle(rows, orows, what)
        _assert_rank0_is_the_result(rows, s.last_results[0], triples[0])
        _assert_order_is_the_rule(L, rows, True)
        nan_t, nan_ml, _, _ = _classes(orows)
        by_idx = _by_index(rows)
        for f in ("ml_score", "ml_confidence", "combined"):      # (assert_allclose above already holds NaN equal to NaN only)
            assert np.isnan(by_idx[f][nan_ml]).all(), (what, f)
        taken_by_ml = rows["index"][rows["by_ml"] == 1].tolist()
        assert not set(taken_by_ml) & (set(nan_ml) | set(nan_t)), (what, taken_by_ml)
        # the plain call: the same result record, and the oracle's triple
        got = s.select_grasp_points_batch(m, d)
        assert bytes(s.last_results) == res_c and got == triples, what
        _same_triple(s.select_grasp_point(_dev(mask), _dev(holed), None), exp)
        raw[hname] = (cands.tobytes(), res_c)
    assert raw["default"] == raw["LG_CNN_PRUNE=0"] == raw["LG_DEFER_PLANES=0"], f"frame {name} {value}: rows of the three handles"


def test_get_ml_score(handles):
    """The mirror method at one candidate of each class against the oracle's ml_post(cnn(patch_features)) over the planes the
    mirror itself computed: NaN where the window holds a hole, the finite score elsewhere."""
    _, orows = _expected("A", "nan")
    mask, _, holed, P, _ = _frame("A", "nan")
    _, nan_ml, fin_ml, _ = _classes(orows)
    s = handles["default"]
    s.set_camera_params(P)
    m8 = mask.astype(np.uint8)
    maps, _, _ = s.score_maps(_dev(m8), _dev(holed))
    maps_np = {k: v.cpu().numpy() for k, v in maps.items()}
    ref = O.RefGraspPointSelector()
    for i, want_nan in ((nan_ml[0], True), (fin_ml[0], False)):
        pt = (orows[i]["x"], orows[i]["y"])
        with np.errstate(all="ignore"):
            feat = ref.patch_features(m8, holed, maps_np, pt)
            exp = ref.ml_post(O.cnn_forward(_params(), feat[None], dtype=torch.float64)[0])
        assert math.isnan(exp) == want_nan, (pt, exp)
        got = s.get_ml_score(_dev(mask), _dev(holed), maps, pt)
        assert got is not None
        if want_nan:
            assert math.isnan(got), (pt, got)
        else:
            assert abs(got - exp) <= 1e-4 and abs(got - orows[i]["ml"]) <= 1e-4, (pt, got, exp, orows[i]["ml"])


def test_batch_isolation(handles):
    """Four frames, one of them holed, against the same batch with that frame's clean version: the other three frames' rows
    and result records are byte-identical."""
    mask, depth, holed, P, _ = _frame("B", "nan")
    H, W = mask.shape
    others = []
    for cx, cy, a, b in ((100, 70, 70, 45), (120, 85, 85, 40), (112, 80, 60, 55)):
        others.append(_ellipse(H, W, cx, cy, a, b))
    masks = np.stack([others[0], mask, others[1], others[2]])
    depths = {k: np.stack([depth, dd, depth, depth]) for k, dd in (("holed", holed), ("clean", depth))}
    for hname, s in handles.items():
        s.set_camera_params(P)
        got = {}
        for k, dd in depths.items():
            _, cands = s.select_grasp_candidates_batch(_dev(masks), _dev(dd))
            rec_c = [bytes(s.last_results)[i * 56:(i + 1) * 56] for i in range(4)]
            s.select_grasp_points_batch(_dev(masks), _dev(dd))
            rec_p = [bytes(s.last_results)[i * 56:(i + 1) * 56] for i in range(4)]
            got[k] = (cands, rec_c, rec_p)
        for b in (0, 2, 3):
            assert got["holed"][0][b].tobytes() == got["clean"][0][b].tobytes(), (hname, b)
            assert got["holed"][1][b] == got["clean"][1][b] and got["holed"][2][b] == got["clean"][2][b], (hname, b)
        rows = _valid_rows(got["holed"][0][1])
        assert np.isnan(rows["ml_score"][rows["scored"] == 1]).any() and got["holed"][0][1].tobytes() != got["clean"][0][1].tobytes()
        assert not np.isnan(_valid_rows(got["clean"][0][1])["ml_score"][_valid_rows(got["clean"][0][1])["scored"] == 1]).any()


# ------------------------------------------------------------------------------------------------- holes off the leaf
# A leaf 7 px tall (rows 60..66) with min_edge_distance 3: only its middle row is valid, so every candidate lies 4 px from the
# rim and an off-leaf pixel up to 12 px from the rim falls inside its window (rows y - 16 .. y + 15).  With the default
# min_edge_distance of 20 no off-leaf pixel can lie in any candidate's window.
OH, OW, BAR_Y0, BAR_Y1, BAR_X0, BAR_X1, MIN_EDGE = 200, 320, 60, 67, 40, 281, 3.0
OFF_RIM = (2, 12, 2, 12)          # distance of the hole above candidates 1, 2, 4, 5 from the leaf's top row
OFF_CANDS = (1, 2, 4, 5)


class _HolesOffLeafRef(O.RefGraspPointSelector):
    """The expectation for holes off the leaf: the planes (and so the candidates and the traditional scores) are those of the
    depth with its non-finite off-leaf pixels set to 1.0 -- quirk 9's deviation -- while patch_features, the 3-D point and
    the pre-grasp point read the raw depth the caller passed."""

    def __init__(self, cnn=None):
        super().__init__(cnn=cnn, params=dict(min_edge_distance=MIN_EDGE))

    def _calculate_all_scores(self, m, depth_f32):
        d = np.asarray(depth_f32, np.float32)
        return super()._calculate_all_scores(m, np.where((np.asarray(m) == 0) & ~np.isfinite(d), np.float32(1.0), d))


@functools.lru_cache(maxsize=None)
def _off_leaf_frame(value):
    """(mask, holed depth, cleaned depth, P, holes)."""
    _, depth, P = O.synthetic_scene(OH, OW, 5)
    mask = np.zeros((OH, OW), bool)
    mask[BAR_Y0:BAR_Y1, BAR_X0:BAR_X1] = True
    ref = _HolesOffLeafRef()
    ref.set_camera_params(P)
    _, dbg = ref.select_grasp_point(mask.astype(np.uint8), depth, mask_is_bool=True, return_debug=True)
    cands = dbg["candidates"]
    d = depth.copy()
    holes = []
    for i, r in zip(OFF_CANDS, OFF_RIM):
        x, y = cands[i]
        assert mask[y, x] and y - 16 <= BAR_Y0 - r
        d[BAR_Y0 - r, x] = VALUES[value]
        holes.append((x, BAR_Y0 - r))
    assert not mask[[h[1] for h in holes], [h[0] for h in holes]].any()
    clean = np.where(~mask & ~np.isfinite(d), np.float32(1.0), d)
    return mask, d, clean, P, holes


@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
def test_holes_off_the_leaf_inside_candidate_windows(L, handles, monkeypatch, value):
    mask, holed, clean, P, holes = _off_leaf_frame(value)
    monkeypatch.setattr(O, "RefGraspPointSelector", _HolesOffLeafRef)      # _oracle_rows builds its selector by this name
    exp, orows = _oracle_rows(P, mask, holed, True, mask_is_bool=True)
    _, orows_clean = _oracle_rows(P, mask, clean, True, mask_is_bool=True)
    monkeypatch.undo()
    # preconditions, from the oracle alone
    nan_t, nan_ml, fin_ml, _ = _classes(orows)
    assert not nan_t and orows[0]["ml"] is not None and not math.isnan(orows[0]["ml"])      # candidate 0 is finite
    assert len(nan_ml) >= 2 and len(fin_ml) >= 2, (nan_ml, fin_ml)
    in_window = [i for i, o in enumerate(orows) if any(-16 <= hx - o["x"] < 16 and -16 <= hy - o["y"] < 16 for hx, hy in holes)]
    assert in_window == nan_ml and {2, 12} == {BAR_Y0 - hy for _, hy in holes}
    assert [(o["x"], o["y"], o["trad"]) for o in orows] == [(o["x"], o["y"], o["trad"]) for o in orows_clean]
    m, dh, dc = _dev(mask[None]), _dev(holed[None]), _dev(clean[None])
    raw = {}
    for hname, s in handles.items():
        s.set_camera_params(P)
        keep = s.min_edge_distance
        s.min_edge_distance = MIN_EDGE
        try:
            maps_h, valid_h, _ = s.score_maps(m, dh)
            maps_c, valid_c, _ = s.score_maps(m, dc)
            triples, cands = s.select_grasp_candidates_batch(m, dh)
            res = s.last_results
            res_c = bytes(res)
            _, cands_c = s.select_grasp_candidates_batch(m, dc)
            plain = s.select_grasp_points_batch(m, dh)
            res_p = bytes(s.last_results)
            one = s.select_grasp_point(_dev(mask), _dev(holed), None)
        finally:
            s.min_edge_distance = keep
        what = f"off the leaf {value}, {hname}"
        # the planes, the candidate list and every traditional score are those of the cleaned frame
        for k in maps_h:
            np.testing.assert_array_equal(maps_h[k].cpu().numpy(), maps_c[k].cpu().numpy(), err_msg=f"{what} {k}")
        np.testing.assert_array_equal(valid_h.cpu().numpy(), valid_c.cpu().numpy())
        rows, rows_c = _valid_rows(cands[0]), _valid_rows(cands_c[0])
        bi, bc = _by_index(rows), _by_index(rows_c)
        for f in ("index", "x", "y", "traditional", "scored", "X", "Y", "Z", "has_pre", "pX", "pY", "pZ"):
            np.testing.assert_array_equal(bi[f], bc[f], err_msg=f"{what} {f}")
        # a candidate with a hole in its window is scored, has NaN ML fields and is never taken by ML; the others keep the
        # values of the cleaned frame
        assert (bi["scored"][nan_ml] == 1).all(), what
        holed_rows = np.zeros(len(bi), bool)
        holed_rows[nan_ml] = True
        for f in ("ml_score", "ml_confidence", "combined"):
            assert np.isnan(bi[f][holed_rows]).all(), (what, f, bi[f][holed_rows])
            np.testing.assert_array_equal(bi[f][~holed_rows].view(np.uint32), bc[f][~holed_rows].view(np.uint32), err_msg=f"{what} {f}")
        assert not set(rows["index"][rows["by_ml"] == 1].tolist()) & set(nan_ml), what
        # the rows against the oracle, the order against the rule, rank 0 against the result and the triple
        _assert_rows_match_oracle(rows, orows, what)
        _assert_order_is_the_rule(L, rows, True)
        _assert_rank0_is_the_result(rows, res[0], triples[0])
        assert plain == triples and res_p == res_c, what
        _same_triple(one, exp)
        raw[hname] = (cands.tobytes(), res_c)
    assert raw["default"] == raw["LG_CNN_PRUNE=0"] == raw["LG_DEFER_PLANES=0"], f"off the leaf {value}: rows of the three handles"
