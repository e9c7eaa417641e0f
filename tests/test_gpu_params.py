"""The constants of lg_params away from the reference's values: the HIP path under every set of tests/param_sets.py against the
oracle built with the same set (oracle.RefParams).  Tolerances are the project's own (BASELINE.json north_star): float planes
rtol 1e-4 / atol 1e-6; distance_map, stem_penalty, valid and candidate pixels bit-exact.  tests/test_oracle_params.py shows on
the CPU that every set moves the output it feeds on its scene (the two 1080 x 1920 pairings included), so nothing here compares
zeros with zeros.
Each test prints the largest tolerance-relative error per float plane, max |got - want| / (|want| + atol / rtol)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import param_oracle as PO  # noqa: E402
from tests import param_sets as PS  # noqa: E402
from tests.test_gpu_grasp_candidates import _assert_rows_match_oracle, _by_index, _valid_rows  # noqa: E402
from tests.test_gpu_headline_batch import _assert_frame_equals_single  # noqa: E402
from tests.test_gpu_parity import ATOL, RTOL, _compare_maps  # noqa: E402
from tests.test_gpu_sparse_planes import _assert_sparse_equals_dense  # noqa: E402

FLOAT_PLANES = ("sdf_score", "approach_score", "flatness_map", "isolation_map", "accessibility_map", "traditional_score")


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


def _selector(L, params, P, shape, with_cnn=False):
    """A fresh selector carrying `params` (a full dict of lg_params fields) and the ImageProcessor that carries its Gaussian size.
    min_edge_distance and gaussian_size go through the attributes the mirror reads; mask_is_bool follows the mask's dtype."""
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_camera_params(P)
    for k, v in params.items():
        if k not in ("min_edge_distance", "gaussian_size", "mask_is_bool"):
            setattr(sel.params, k, v)
    sel.min_edge_distance = params["min_edge_distance"]
    if with_cnn:
        sel.set_cnn_state_dict(PO.cnn_params())
    return sel, L.ImageProcessor(shape[0], shape[1], 21, params["gaussian_size"])


def _mask_tensor(mask, params):
    m = torch.from_numpy(np.ascontiguousarray(mask))
    return (m != 0).cuda() if params["mask_is_bool"] else m.cuda()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _report(what, maps, sc):
    figs = {k: float(np.max(np.abs(maps[k].cpu().numpy().astype(np.float64) - sc[k]) / (np.abs(sc[k]) + ATOL / RTOL)))
            for k in FLOAT_PLANES}
    print(f"PLANE-ERRORS {what}: " + " ".join(f"{k}={v:.3g}" for k, v in figs.items()))


def _planes_and_candidates(L, name, scene):
    ps = PS.BY_NAME[name]
    params = PS.params_of(ps)
    mask, depth, P = PO.scene(scene)
    sel, ip = _selector(L, params, P, mask.shape)
    ref = PO.oracle(P, params)
    maps, valid, sc = _compare_maps(sel, mask, depth, P, ref=ref, image_processor=ip)
    _report(f"{name} on {scene}", maps, sc)
    # the candidates: integer work on identical inputs -- the oracle's walk over the DEVICE's planes, the set's top_k / spacing
    k, md = params["top_k"], params["nms_min_distance"]
    got = sel._get_candidate_points(maps["traditional_score"], valid, k, md)
    want = ref._get_candidate_points(maps["traditional_score"].cpu().numpy(), valid.cpu().numpy().astype(bool), k, md)
    assert got == want and (len(got) == k or not mask.any())
    # ... and the candidates the whole call produces for itself: lg_params.top_k / nms_min_distance read by the pipeline, its own
    # planes and validity (unwritten on constant tiles), the per-tile maxima
    _, cands = sel.select_grasp_candidates_batch(_mask_tensor(mask, params), _dev(depth), image_processor=ip, top_k=k)
    rows = _by_index(_valid_rows(cands[0]))
    assert [(int(r["x"]), int(r["y"])) for r in rows] == want
    return sel


@pytest.mark.parametrize("name", [s.name for s in PS.SETS])
def test_planes_and_candidates_vs_oracle(L, name):
    _planes_and_candidates(L, name, PS.BY_NAME[name].scene)


# ----------------------------------------------------------------------------- sparse and dense forms
@functools.lru_cache(maxsize=None)
def _batch(shape, n):
    """n frames of one shape: the largest leaf of n - 1 seeded scenes and an empty mask"""
    H, W = shape
    scenes = [PO.scene((H, W, 30 + i, "largest")) for i in range(n - 1)]
    masks = np.stack([s[0] for s in scenes] + [np.zeros((H, W), np.uint8)]).astype(bool)
    depth = np.stack([s[1] for s in scenes] + [scenes[0][1]])
    return masks, depth


@pytest.mark.parametrize("name", PS.SPARSE_DENSE)
def test_sparse_rows_equal_dense_rows(L, name):
    """lg_final_kernel, lg_topk_kernel and lg_gather_kernel each compute the constant tile's value w_flat * flatness(flat_scale)
    for themselves: without plane outputs the three must agree to the bit, or the rows differ from the dense call's."""
    ps = PS.BY_NAME[name]
    params = PS.params_of(ps)
    mask, depth, P = PO.scene(ps.scene)
    sel, ip = _selector(L, params, P, mask.shape, with_cnn=True)
    masks, depths = _batch(mask.shape, 8)
    masks = np.concatenate([masks, mask[None].astype(bool)])
    depths = np.concatenate([depths, depth[None]])
    sel.select_grasp_points_batch = functools.partial(sel.select_grasp_points_batch, image_processor=ip)
    triples = _assert_sparse_equals_dense(sel, masks, depths)
    H, W = mask.shape
    # no valid pixel (the empty mask; every frame where nothing is valid): the walk falls through to the frame's last pixel
    assert len(triples) == 9 and triples[7][0] == (W - 1, H - 1) and all(t[0] is not None for t in triples)
    if name not in ("stem_valid_thresh=0", "negative_approach"):
        assert sum(t[0] != (W - 1, H - 1) for t in triples) >= 6
    exp = PO.run_set(name, True)["triple"] if name in PS.END_TO_END else None
    if exp is not None:
        assert triples[8][0] == exp[0]


# ----------------------------------------------------------------------------- the whole selection
def _oracle_rows(r, depth, mask):
    rows = []
    ml = r["ml_scores"] or [None] * len(r["candidates"])
    for (x, y), m, pre in zip(r["candidates"], ml, r["pregrasp"]):
        t = float(r["scores"]["traditional_score"][y, x])
        conf = comb = None
        if m is not None:
            conf = 1.0 - abs(m - 0.5) * 2
            w = min(0.3, conf * 0.6)
            comb = (1.0 - w) * t + w * m
        rows.append(dict(x=x, y=y, trad=t, ml=m, conf=conf, comb=comb, g3=r["ref"].get_3d_grasp_point((x, y), depth), pre=pre))
    return rows


def _assert_triple(got, exp):
    assert got[0] == exp[0], (got, exp)
    np.testing.assert_allclose(got[1], exp[1], rtol=1e-5)
    assert (got[2] is None) == (exp[2] is None)
    if exp[2] is not None:
        np.testing.assert_allclose(got[2], exp[2], rtol=1e-5)


@pytest.mark.parametrize("with_cnn", [False, True])
@pytest.mark.parametrize("name", PS.END_TO_END)
def test_selection_vs_oracle(L, name, with_cnn):
    """select_grasp_point and select_grasp_candidates against the oracle's own selection (its planes, its candidates, its pick)
    on scenes without near-ties (tests/test_oracle_params.py::test_end_to_end_scenes_have_no_near_tie)."""
    ps = PS.BY_NAME[name]
    params = PS.params_of(ps)
    mask, depth, P = PO.scene(ps.scene)
    exp = PO.run_set(name, with_cnn)
    sel, ip = _selector(L, params, P, mask.shape, with_cnn=with_cnn)
    m, d = _mask_tensor(mask, params), _dev(depth)
    got = sel.select_grasp_point(m, d, ip)
    _assert_triple(got, exp["triple"])
    triples, cands = sel.select_grasp_candidates_batch(m, d, image_processor=ip, top_k=params["top_k"])
    _assert_triple(triples[0], exp["triple"])
    rows = _valid_rows(cands[0])
    _assert_rows_match_oracle(rows, _oracle_rows(exp, depth, mask), name)
    assert (int(rows[0]["x"]), int(rows[0]["y"])) == exp["triple"][0]
    listed = sel.select_grasp_candidates(m, d, ip, top_k=params["top_k"])
    assert sorted((c["index"], c["point_2d"]) for c in listed) == list(enumerate(exp["candidates"]))
    if params["top_k"] == 1:
        assert not rows["scored"].any()          # no rescoring of a single candidate (:208 len(candidates) > 1)
    elif with_cnn and not params["mask_is_bool"]:
        assert rows["scored"].all()              # a uint8 mask: border candidates are scored too
    if name == "negative_approach":              # every valid pixel is below zero: the walk hands out invalid pixels
        assert not any(exp["valid"][y, x] for x, y in exp["candidates"])


# ----------------------------------------------------------------------------- pre-grasp
@pytest.mark.parametrize("scene", ["offaxis", "top_strip"])
@pytest.mark.parametrize("clearance", [0, 1, 30, 31])
def test_pregrasp_clearance_vs_oracle(L, clearance, scene):
    """calculate_pre_grasp_point with the (2 c + 1) ellipse at both ends of its range, for a pick mid-frame and for picks within
    31 px of the frame border (where the ellipse hangs over the edge).  Every row's pre-grasp point against the oracle's AT THE
    DEVICE's OWN candidates, and the returned triple's against the oracle's at the returned point."""
    name = f"pregrasp_clearance={clearance}" + ("_at_the_border" if scene == "top_strip" else "")
    ps = PS.BY_NAME[name]
    assert ps.scene == scene
    params = PS.params_of(ps)
    mask, depth, P = PO.scene(scene)
    sel, ip = _selector(L, params, P, mask.shape)
    ref = PO.oracle(P, params)
    ref15 = PO.oracle(P, dict(params, pregrasp_clearance=15))
    triples, cands = sel.select_grasp_candidates_batch(_mask_tensor(mask, params), _dev(depth), image_processor=ip)
    rows = _by_index(_valid_rows(cands[0]))
    assert len(rows) == 20
    moved = 0
    H, W = mask.shape
    for r in rows:
        pt = (int(r["x"]), int(r["y"]))
        g3 = ref.get_3d_grasp_point(pt, depth)
        want = ref.calculate_pre_grasp_point(g3, mask)
        assert want is not None and r["has_pre"]
        np.testing.assert_allclose([r["pX"], r["pY"], r["pZ"]], want, rtol=1e-5, atol=1e-9, err_msg=f"{name} {pt}")
        moved += want != ref15.calculate_pre_grasp_point(g3, mask)
    (x, y), _, pre = triples[0]
    edge = min(x, y, W - 1 - x, H - 1 - y)
    assert edge <= 31 if scene == "top_strip" else edge > 100
    np.testing.assert_allclose(pre, ref.calculate_pre_grasp_point(ref.get_3d_grasp_point((x, y), depth), mask), rtol=1e-5)
    assert moved >= 1, "the clearance must decide at least one of the frame's pre-grasp points"


# ----------------------------------------------------------------------------- batch = single, and nothing survives a call
def _call(sel, ip, masks, depths, top_k):
    maps, valid, _ = sel.score_maps(_dev(masks), _dev(depths), ip)
    triples, cands = sel.select_grasp_candidates_batch(_dev(masks), _dev(depths), image_processor=ip, top_k=top_k)
    return {k: v.cpu().numpy() for k, v in maps.items()}, valid.cpu().numpy(), triples, cands


def test_batch_of_16_equals_single_calls_under_an_all_different_set(L):
    ps = PS.BY_NAME["all_different_a"]
    params = PS.params_of(ps)
    H, W = 200, 1028
    masks, depths = _batch((H, W), 16)
    P = PO.scene(ps.scene)[2]
    sel, ip = _selector(L, params, P, (H, W), with_cnn=True)
    maps, valid, triples, cands = _call(sel, ip, masks, depths, params["top_k"])
    differ = 0
    for b in range(16):
        m1, v1, t1, c1 = _call(sel, ip, masks[b][None], depths[b][None], params["top_k"])
        for k in maps:
            np.testing.assert_array_equal(maps[k][b], m1[k][0], err_msg=f"{k} frame {b}")
        np.testing.assert_array_equal(valid[b], v1[0])
        rb, rs = _valid_rows(cands[b]), _valid_rows(c1[0])
        differ += _assert_frame_equals_single(rb, rs, f"frame {b}")
        if len(rb) and rb["index"][0] == rs["index"][0]:
            assert triples[b] == t1[0], b
    assert all(t[0] is not None for t in triples) and triples[15][0] == (W - 1, H - 1)   # (the empty mask falls through)
    print(f"16 frames under all_different_a: {differ} frames whose rank order differs at a near-tie")


def test_consecutive_calls_with_different_sets_equal_fresh_handles(L):
    """Nothing derived from the previous call's parameters (SE spans, 1 / (2 opt^2), the ramp step, the workspace sized by top_k)
    may survive on a handle."""
    H, W = 200, 1028
    masks, depths = _batch((H, W), 4)
    P = PO.scene("cut")[2]
    names = ["all_different_b", "all_different_a", "stem_se=64", "gauss1_top1", "intmax_top64_nms25", "negative_approach",
             "all_different_b"]
    used, _ = _selector(L, PS.params_of({}), P, (H, W), with_cnn=True)
    for name in names:
        params = PS.params_of(name)
        fresh, ip = _selector(L, params, P, (H, W), with_cnn=True)
        for k, v in params.items():
            if k not in ("min_edge_distance", "gaussian_size", "mask_is_bool"):
                setattr(used.params, k, v)
        used.min_edge_distance = params["min_edge_distance"]
        a = _call(used, ip, masks, depths, params["top_k"])
        b = _call(fresh, ip, masks, depths, params["top_k"])
        for k in a[0]:
            np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=f"{name} {k}")
        np.testing.assert_array_equal(a[1], b[1], err_msg=name)
        assert a[2] == b[2], name
        assert a[3].tobytes() == b[3].tobytes(), name


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("field,value", PS.REFUSED)
def test_out_of_range_constants_are_refused(L, field, value):
    mask, depth, P = PO.scene("cut")
    sel, ip = _selector(L, PS.params_of({}), P, mask.shape)
    m, d = _mask_tensor(mask, PS.DEFAULTS), _dev(depth)
    setattr(sel.params, field, value)
    with pytest.raises(L.LgError, match="status -1"):      # LG_ERR_INVALID
        sel.select_grasp_points_batch(m, d)
    assert sel.select_grasp_point(m, d, None) == (None, None, None)   # through the mirror: the reference-style None triple
    setattr(sel.params, field, PS.DEFAULTS[field])
    _assert_triple(sel.select_grasp_point(m, d, None), PO.run(PS.params_of({}), "cut")["triple"])
    _compare_maps(sel, mask, depth, P)
