"""Ranked grasp candidates on the device (lg_select_grasp_candidates, lg_candidates_kernel) against the float64 oracle: every
candidate's scores, 3-D and pre-grasp point, the rank order (the reference's selection applied again to what is left), rank 0
against lg_select_grasp, and the edge cases.  1080 x 1920 with the CNN unless a test says otherwise."""
import ctypes as C
import functools
import math

import numpy as np
import numpy.lib.recfunctions as rfn
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

H, W = 1080, 1920


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


@pytest.fixture(scope="module")
def sel(L):
    return L.GraspPointSelector(torch.device("cuda:0"), load_model=False)


@functools.lru_cache(maxsize=None)
def _params():
    return O.cnn_closed_form_params(seed=0)


@functools.lru_cache(maxsize=None)
def _scene(seed):
    labels, depth, P = O.synthetic_scene(H, W, seed)
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    leaf = int(ids[np.argmax(counts)])
    return labels, labels == leaf, depth, P, leaf


def _cnn(sel, on):
    if on:
        sel.set_cnn_state_dict(_params())
    else:
        sel.clear_cnn()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle_rows(P, mask, depth, with_cnn, mask_is_bool=True):
    """The oracle's candidate list with the values the reference logs for each candidate (:210-236), its 3-D and pre-grasp point."""
    ref = O.RefGraspPointSelector(cnn=(lambda x: O.cnn_forward(_params(), x)) if with_cnn else None)
    ref.set_camera_params(P)
    m8 = np.ascontiguousarray(mask, np.uint8)
    with np.errstate(all="ignore"):
        exp, dbg = ref.select_grasp_point(m8, depth, mask_is_bool=mask_is_bool, return_debug=True)
        cands = dbg.get("candidates", [])
        ml = dbg.get("ml_scores") or [None] * len(cands)
        rows = []
        for i, (x, y) in enumerate(cands):
            t = float(dbg["scores"]["traditional_score"][y, x])
            m = ml[i]
            conf = comb = None
            if m is not None:
                conf = 1.0 - abs(m - 0.5) * 2
                w = min(0.3, conf * 0.6)
                comb = (1.0 - w) * t + w * m
            g3 = ref.get_3d_grasp_point((x, y), depth)
            rows.append(dict(x=x, y=y, trad=t, ml=m, conf=conf, comb=comb, g3=g3, pre=ref.calculate_pre_grasp_point(g3, m8)))
    return exp, rows


def _valid_rows(c):
    n = int((c["index"] >= 0).sum())
    assert (c["index"][:n] >= 0).all() and (c["index"][n:] == -1).all()
    tail = c[n:].copy()
    tail["index"] = 0
    assert tail.tobytes() == bytes(tail.nbytes), "rows past n_candidates must be zeros"
    return c[:n]


def _by_index(rows):
    return rows[np.argsort(rows["index"], kind="stable")]


def _assert_rows_match_oracle(rows, orows, what=""):
    rows = _by_index(rows)
    assert rows["index"].tolist() == list(range(len(orows))), what
    assert [(int(r["x"]), int(r["y"])) for r in rows] == [(o["x"], o["y"]) for o in orows], what
    np.testing.assert_allclose(rows["traditional"], [o["trad"] for o in orows], rtol=1e-4, atol=1e-6, equal_nan=True,
                               err_msg=what)
    scored = np.array([o["ml"] is not None for o in orows])
    np.testing.assert_array_equal(rows["scored"].astype(bool), scored, err_msg=what)
    for f, k in (("ml_score", "ml"), ("ml_confidence", "conf"), ("combined", "comb")):
        assert np.isnan(rows[f][~scored]).all(), (what, f)
        np.testing.assert_allclose(rows[f][scored], [o[k] for o in orows if o["ml"] is not None], rtol=0, atol=1e-4,
                                   err_msg=f"{what} {f}")
    np.testing.assert_allclose(np.stack([rows["X"], rows["Y"], rows["Z"]], 1).astype(np.float64),
                               np.array([o["g3"] for o in orows], np.float64), rtol=1e-5, atol=1e-9, equal_nan=True, err_msg=what)
    has_pre = np.array([o["pre"] is not None for o in orows])
    np.testing.assert_array_equal(rows["has_pre"].astype(bool), has_pre, err_msg=what)
    if has_pre.any():
        np.testing.assert_allclose(np.stack([rows["pX"], rows["pY"], rows["pZ"]], 1)[has_pre].astype(np.float64),
                                   np.array([o["pre"] for o in orows if o["pre"] is not None], np.float64), rtol=1e-5,
                                   atol=1e-9, err_msg=what)
    assert (rows["pX"][~has_pre] == 0).all() and (rows["pZ"][~has_pre] == 0).all()


def _rank_step(L, trad, comb, scored, remaining, rescoring):
    """One pick of lg_rank_grasp_candidates over the remaining candidates (candidate order): (candidate, pick score, by_ml)."""
    rem = sorted(remaining)
    n = len(rem)
    t = np.ascontiguousarray([trad[i] for i in rem], np.float64)
    c = np.ascontiguousarray([comb[i] for i in rem], np.float64)
    s = np.ascontiguousarray([scored[i] for i in rem], np.int32)
    o, p, b = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32)
    assert L.lib.lg_rank_grasp_candidates(t.ctypes.data, c.ctypes.data, s.ctypes.data, n, int(rescoring), o.ctypes.data,
                                          p.ctypes.data, b.ctypes.data) == 0
    return rem[int(o[0])], float(p[0]), int(b[0])


def _assert_order_is_the_rule(L, rows, rescoring):
    """The device order equals lg_rank_grasp_candidates on the device's own reported (float32) values.  Allowed: a swap between
    picks whose deciding scores are equal once rounded to float32 (the kernel ranks on the unrounded doubles).  Returns the
    number of such swaps."""
    n = len(rows)
    by_idx = _by_index(rows)
    trad = by_idx["traditional"].astype(np.float64)
    comb = by_idx["combined"].astype(np.float64)
    scored = by_idx["scored"].tolist()
    remaining = set(range(n))
    swaps = 0
    for r in range(n):
        d = int(rows["index"][r])
        best, bs, ml = _rank_step(L, trad, comb, scored, remaining, rescoring and n > 1)
        dv = np.float32(rows["pick_score"][r])
        same_bits = dv.view(np.uint32) == np.float32(bs).view(np.uint32)
        if d != best:
            own = comb[d] if rows["by_ml"][r] else trad[d]
            assert np.float32(own) == np.float32(bs) and dv == np.float32(bs), (r, d, best, own, bs)
            swaps += 1
        else:
            assert same_bits or (math.isnan(bs) and np.isnan(dv)), (r, d, float(dv), bs)
            assert int(rows["by_ml"][r]) == ml or np.float32(comb[d]) == np.float32(trad[d]), (r, d)
        remaining.discard(d)
    return swaps


def _oracle_order_agrees(rows, orows, rescoring, margin):
    """The device order equals the oracle's successive picks wherever the deciding margin (the winner's score minus the best
    score of any other candidate in that pick) exceeds `margin`; the comparison ends at the first pick closer than that which
    resolves differently (the remaining sets differ from there on).  Returns the number of ranks compared."""
    remaining = list(range(len(orows)))
    for r in range(len(rows)):
        j = remaining[0]
        entries = [(orows[j]["trad"], j)]
        if rescoring and len(remaining) > 1:
            entries += [(orows[i]["comb"], i) for i in remaining if orows[i]["comb"] is not None]
        bs, best = entries[0]
        for v, i in entries[1:]:
            if v > bs:
                bs, best = v, i
        others = [v for v, i in entries if i != best and not math.isnan(v)]
        gap = math.inf if math.isnan(bs) or not others else bs - max(others)
        d = int(rows["index"][r])
        if d != best:
            assert gap <= margin, (r, d, best, gap)
            return r
        assert math.isclose(float(rows["pick_score"][r]), bs, rel_tol=0, abs_tol=1e-4) or (math.isnan(bs) and np.isnan(rows["pick_score"][r]))
        remaining.remove(best)
    return len(rows)


def _assert_rank0_is_the_result(rows, res, triple):
    assert res.found == 1 and res.n_candidates == len(rows)
    r0 = rows[0]
    assert (int(r0["x"]), int(r0["y"])) == (res.x, res.y) == tuple(triple[0])
    f32 = lambda v: np.float32(v).view(np.uint32)  # noqa: E731
    for a, b in (("X", "X"), ("Y", "Y"), ("Z", "Z"), ("pX", "pX"), ("pY", "pY"), ("pZ", "pZ"), ("pick_score", "best_score")):
        assert f32(r0[a]) == f32(getattr(res, b)), (a, r0[a], getattr(res, b))
    assert int(r0["has_pre"]) == res.has_pre and int(r0["by_ml"]) == res.ml_used


# ----------------------------------------------------------------------------- against the oracle
def test_rows_and_order_against_the_oracle_1080p(L, sel):
    """Seeds 22 and 23 (interior leaves, every candidate strictly positive) and 21 (the whole leaf under the stem penalty: the
    zero-score fall-through), with the CNN, in one batch."""
    seeds = [22, 23, 21]
    frames = [_scene(s) for s in seeds]
    P = frames[0][3]
    sel.set_camera_params(P)
    _cnn(sel, True)
    masks = _dev(np.stack([f[1] for f in frames]))
    depths = _dev(np.stack([f[2] for f in frames]))
    triples = sel.select_grasp_points_batch(masks, depths)
    res_plain = bytes(sel.last_results)
    triples2, cands = sel.select_grasp_candidates_batch(masks, depths)
    assert bytes(sel.last_results) == res_plain            # results of the candidates entry == lg_select_grasp's, bit for bit
    assert triples2 == triples
    assert cands.shape == (3, 20) and cands.dtype == L.GRASP_CANDIDATE_DTYPE
    for b, (labels, mask, depth, Pb, _) in enumerate(frames):
        rows = _valid_rows(cands[b])
        assert len(rows) == 20
        _assert_rank0_is_the_result(rows, sel.last_results[b], triples[b])
        exp, orows = _oracle_rows(Pb, mask, depth, True)
        _assert_rows_match_oracle(rows, orows, f"seed {seeds[b]}")
        if seeds[b] != 21:   # interior leaves: every candidate is scored (seed 21's fall-through points lie on the frame border)
            assert (rows["scored"] == 1).all()
        assert _assert_order_is_the_rule(L, rows, True) <= 2
        assert _oracle_order_agrees(rows, orows, True, 1e-4) >= 1
        assert (int(rows[0]["x"]), int(rows[0]["y"])) == tuple(exp[0])
    sel.clear_cnn()


def test_without_the_cnn_rank_is_the_candidate_order(L, sel):
    labels, mask, depth, P, _ = _scene(22)
    sel.set_camera_params(P)
    _cnn(sel, False)
    triples, cands = sel.select_grasp_candidates_batch(_dev(mask[None]), _dev(depth[None]))
    rows = _valid_rows(cands[0])
    assert rows["index"].tolist() == list(range(20))
    for f in ("ml_score", "ml_confidence", "combined"):
        assert np.isnan(rows[f]).all()
    assert (rows["scored"] == 0).all() and (rows["by_ml"] == 0).all()
    np.testing.assert_array_equal(rows["pick_score"], rows["traditional"])
    _assert_rank0_is_the_result(rows, sel.last_results[0], triples[0])
    _, orows = _oracle_rows(P, mask, depth, False)
    _assert_rows_match_oracle(rows, orows, "no cnn")


def test_empty_mask_gives_the_fall_through_rows_and_none_leaf_gives_none(L, sel):
    """An empty mask: the reference's candidate list is the zero-score fall-through (the build's total order), so the rows are
    those 20 points, each with its own 3-D point.  A None leaf id (the node makes no select_grasp_point call) gives no rows."""
    labels, mask, depth, P, leaf = _scene(22)
    sel.set_camera_params(P)
    _cnn(sel, True)
    empty = np.zeros_like(mask)
    triples, cands = sel.select_grasp_candidates_batch(_dev(empty[None]), _dev(depth[None]))
    rows = _valid_rows(cands[0])
    _, orows = _oracle_rows(P, empty, depth, True)
    _assert_rows_match_oracle(rows, orows, "empty")
    _assert_rank0_is_the_result(rows, sel.last_results[0], triples[0])
    lab = _dev(np.stack([labels, labels]).astype(np.int16))
    dd = _dev(np.stack([depth, depth]))
    t2, c2 = sel.select_grasp_candidates_for_leaves(lab, [None, leaf], dd)
    assert t2[0] == (None, None, None) and sel.last_results[0].found == 0
    assert (c2[0]["index"] == -1).all() and len(_valid_rows(c2[0])) == 0
    assert len(_valid_rows(c2[1])) == 20
    sel.clear_cnn()


def test_one_candidate_gives_one_unscored_row(L, sel):
    labels, mask, depth, P, _ = _scene(23)
    sel.set_camera_params(P)
    _cnn(sel, True)
    old = sel.params.nms_min_distance
    sel.params.nms_min_distance = 4000       # the suppression window covers the frame: one candidate
    try:
        triples = sel.select_grasp_points_batch(_dev(mask[None]), _dev(depth[None]))
        plain = bytes(sel.last_results)
        t2, cands = sel.select_grasp_candidates_batch(_dev(mask[None]), _dev(depth[None]))
    finally:
        sel.params.nms_min_distance = old
    assert bytes(sel.last_results) == plain and t2 == triples
    rows = _valid_rows(cands[0])
    assert len(rows) == 1 and int(rows[0]["index"]) == 0
    assert rows[0]["scored"] == 0 and rows[0]["by_ml"] == 0 and np.isnan(rows[0]["ml_score"])
    assert rows[0]["pick_score"] == rows[0]["traditional"]
    _assert_rank0_is_the_result(rows, sel.last_results[0], triples[0])
    sel.clear_cnn()


def test_bool_mask_border_candidates_are_unscored(L, sel):
    """A leaf strip along the left frame border: candidates closer than 16 px to the border have no ML score with a torch.bool
    mask and one with a uint8 mask."""
    labels, _, depth, P, _ = _scene(22)
    yy, xx = np.mgrid[:H, :W]
    strip = (xx < 80) & (yy >= 100) & (yy < 600)
    sel.set_camera_params(P)
    _cnn(sel, True)
    _, cb = sel.select_grasp_candidates_batch(_dev(strip[None]), _dev(depth[None]))
    _, cu = sel.select_grasp_candidates_batch(_dev(strip[None].astype(np.uint8)), _dev(depth[None]))
    rb, ru = _by_index(_valid_rows(cb[0])), _by_index(_valid_rows(cu[0]))
    border = (rb["x"] < 16) | (rb["y"] < 16) | (rb["x"] + 16 > W) | (rb["y"] + 16 > H)
    assert border.any() and (~border).any()
    np.testing.assert_array_equal(rb["scored"] == 0, border)
    assert (ru["scored"] == 1).all()
    _, orows = _oracle_rows(P, strip, depth, True, mask_is_bool=True)
    _assert_rows_match_oracle(rb, orows, "bool strip")
    _, orows_u = _oracle_rows(P, strip, depth, True, mask_is_bool=False)
    _assert_rows_match_oracle(ru, orows_u, "uint8 strip")
    sel.clear_cnn()


def test_nan_depth_on_the_leaf(L, sel):
    """NaN depth pixels on the leaf: NaN traditional scores lead the candidate list (NaN first), a NaN start
    is never beaten, and the candidate on the NaN pixel itself has NaN coordinates and no pre-grasp point.  A leaf in the frame's
    last rows and columns, so that the NaN reach of pixel (H-1, W-1) ends at that pixel and it leads the list.  Without the CNN."""
    labels, _, depth, P, _ = _scene(22)
    mask = np.zeros((H, W), bool)
    mask[H - 150:, W - 200:] = True
    d = depth.copy()
    for (y, x) in [(H - 1, W - 1), (H - 60, W - 70)]:
        d[y, x] = np.nan
    sel.set_camera_params(P)
    _cnn(sel, False)
    triples, cands = sel.select_grasp_candidates_batch(_dev(mask[None]), _dev(d[None]))
    rows = _valid_rows(cands[0])
    _, orows = _oracle_rows(P, mask, d, False)
    _assert_rows_match_oracle(rows, orows, "nan depth")
    assert np.isnan(rows["traditional"][0]) and np.isnan(rows["pick_score"][0])
    nan_z = np.isnan(rows["Z"])
    assert nan_z.any() and (rows["has_pre"][nan_z] == 0).all()
    _assert_rank0_is_the_result(rows, sel.last_results[0], triples[0])


@pytest.mark.parametrize("top_k", [1, 64])
def test_top_k_1_and_64(L, sel, top_k):
    labels, mask, depth, P, _ = _scene(22)
    sel.set_camera_params(P)
    _cnn(sel, True)
    m, d = _dev(mask[None]), _dev(depth[None])
    old = sel.params.top_k
    sel.params.top_k = top_k
    try:
        triples = sel.select_grasp_points_batch(m, d)
        plain = bytes(sel.last_results)
    finally:
        sel.params.top_k = old
    t2, cands = sel.select_grasp_candidates_batch(m, d, top_k=top_k)
    assert sel.params.top_k == old
    assert cands.shape == (1, top_k) and bytes(sel.last_results) == plain and t2 == triples
    rows = _valid_rows(cands[0])
    assert len(rows) == top_k
    _assert_rank0_is_the_result(rows, sel.last_results[0], triples[0])
    _assert_order_is_the_rule(L, rows, top_k > 1)
    _, c20 = sel.select_grasp_candidates_batch(m, d)
    first = _by_index(rows)[:min(top_k, 20)]                  # greedy spaced top-k: a longer list extends the shorter one
    r20 = _by_index(_valid_rows(c20[0]))[:min(top_k, 20)]
    keep = ["index", "x", "y", "traditional", "X", "Y", "Z", "has_pre", "pX", "pY", "pZ"]
    assert rfn.repack_fields(first[keep]).tobytes() == rfn.repack_fields(r20[keep]).tobytes()
    for bad in (0, 65):
        with pytest.raises(ValueError):
            sel.select_grasp_candidates_batch(m, d, top_k=bad)
    sel.clear_cnn()


def test_labels_entry_equals_masks_entry(L, sel):
    seeds = [22, 23]
    frames = [_scene(s) for s in seeds]
    sel.set_camera_params(frames[0][3])
    _cnn(sel, True)
    lab = _dev(np.stack([f[0] for f in frames]).astype(np.int16))
    depths = _dev(np.stack([f[2] for f in frames]))
    ids = [f[4] for f in frames]
    t_lab, c_lab = sel.select_grasp_candidates_for_leaves(lab, ids, depths)
    r_lab = bytes(sel.last_results)
    t_msk, c_msk = sel.select_grasp_candidates_batch(_dev(np.stack([f[1] for f in frames])), depths)
    assert t_lab == t_msk and c_lab.tobytes() == c_msk.tobytes() and r_lab == bytes(sel.last_results)
    assert sel.select_grasp_points_for_leaves(lab, ids, depths) == t_lab
    sel.clear_cnn()


def _mixed_frames():
    """Seven 1080p frames: interior leaves, the fall-through leaf, an empty mask, a border strip, NaN depth on a leaf."""
    out = []
    for s in (22, 23, 21):
        _, mask, depth, P, _ = _scene(s)
        out.append((mask, depth))
    _, mask, depth, P, _ = _scene(22)
    out.append((np.zeros_like(mask), depth))
    yy, xx = np.mgrid[:H, :W]
    out.append(((xx < 80) & (yy >= 100) & (yy < 600), depth))
    d = depth.copy()
    ys, xs = np.nonzero(mask)
    d[int(ys.mean()), int(xs.mean())] = np.nan
    out.append((mask, d))
    _, mask24, depth24, _, _ = _scene(24)
    out.append((mask24, depth24))
    return out, P


@pytest.mark.parametrize("with_cnn", [False, True])
def test_batch_of_seven_equals_single_calls(L, sel, with_cnn):
    frames, P = _mixed_frames()
    assert len(frames) == 7
    sel.set_camera_params(P)
    _cnn(sel, with_cnn)
    masks = _dev(np.stack([f[0] for f in frames]))
    depths = _dev(np.stack([f[1] for f in frames]))
    tb, cb = sel.select_grasp_candidates_batch(masks, depths)
    for b, (mask, depth) in enumerate(frames):
        ts, cs = sel.select_grasp_candidates_batch(_dev(mask[None]), _dev(depth[None]))
        if not with_cnn:
            assert cb[b].tobytes() == cs[0].tobytes(), b
            continue
        rb, rs = _valid_rows(cb[b]), _valid_rows(cs[0])
        assert len(rb) == len(rs)
        xb, xs_ = _by_index(rb), _by_index(rs)
        for f in ("index", "x", "y", "traditional", "scored", "X", "Y", "Z", "has_pre", "pX", "pY", "pZ"):
            np.testing.assert_array_equal(xb[f], xs_[f], err_msg=f"{b} {f}")
        for f in ("ml_score", "ml_confidence", "combined"):
            np.testing.assert_allclose(xb[f], xs_[f], rtol=1e-5, equal_nan=True, err_msg=f"{b} {f}")
        # the order matches wherever the deciding margins (of the single call's values) exceed 1e-5
        orows = [dict(trad=float(r["traditional"]), comb=None if not r["scored"] else float(r["combined"])) for r in xs_]
        _oracle_order_agrees(rb, orows, len(rb) > 1, 1e-5)
    sel.clear_cnn()


def test_existing_calls_do_not_launch_the_candidates_kernel(L, sel):
    labels, mask, depth, P, leaf = _scene(22)
    sel.set_camera_params(P)
    _cnn(sel, True)
    lab = _dev(labels[None].astype(np.int16))
    d = _dev(depth[None])

    def launches():
        n, ms = C.c_int(-1), C.c_double(0.0)
        assert L.lib.lg_profile_read(sel._h, b"candidates", C.byref(n), C.byref(ms)) == 0
        return n.value

    assert L.lib.lg_profile_enable(sel._h, 1) == 0
    try:
        sel.select_grasp_points_batch(_dev(mask[None]), d)
        sel.select_grasp_points_for_leaves(lab, [leaf], d)
        assert launches() == 0
        sel.select_grasp_candidates_batch(_dev(mask[None]), d)
        assert launches() == 1
    finally:
        L.lib.lg_profile_enable(sel._h, 0)
    sel.clear_cnn()


def test_single_frame_dicts(L, sel):
    labels, mask, depth, P, _ = _scene(22)
    sel.set_camera_params(P)
    _cnn(sel, True)
    got = sel.select_grasp_candidates(torch.from_numpy(mask).cuda(), torch.from_numpy(depth).cuda())
    best = sel.select_grasp_point(torch.from_numpy(mask).cuda(), torch.from_numpy(depth).cuda(), None)
    assert len(got) == 20 and sorted(g["index"] for g in got) == list(range(20))
    assert (got[0]["point_2d"], got[0]["point_3d"], got[0]["pre_grasp_point"]) == best
    for g in got:
        for k in L.GRASP_CANDIDATE_DTYPE.names:
            assert k in g
        assert isinstance(g["point_2d"][0], int) and isinstance(g["point_3d"][0], float)
        assert (g["ml_score"] is None) == (not g["scored"])
    sel.clear_cnn()
    assert all(g["ml_score"] is None and g["combined"] is None
               for g in sel.select_grasp_candidates(torch.from_numpy(mask).cuda(), torch.from_numpy(depth).cuda()))
    # never raises: no camera parameters -> logged, []
    fresh = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    assert fresh.select_grasp_candidates(torch.from_numpy(mask).cuda(), torch.from_numpy(depth).cuda()) == []
