"""The whole selection at the smallest, widest and tallest frames make_plan admits (tests/frame_shapes.py), against the oracle:
float planes rtol 1e-4 / atol 1e-6, distance_map, stem_penalty, valid, the candidate pixels and the 16.16 isolation fields bit
for bit, triples rtol 1e-5 -- the project's own tolerances, through the helpers of the tests that set them.
tests/test_frame_shapes_host.py shows on the CPU that every case has valid pixels and no near-tie.

Paths that no other test reaches, and the test here that asserts each was reached:
  lg_dt5_kernel<1024, 8, *, *> (4096 < W <= 8192)         test_wide_and_tall_frames_vs_oracle[24x4160 / 24x8192 / 8x8192-sweeps]
  lg_hrun_kernel's 64-word pieces (a box wider than 64 words) test_wide_and_tall_frames_vs_oracle[24x4160 ... -search1 / bands]
  lg_iso_sweep_kernel<32, *> (W > 2048)                      test_label_aware_fields_and_plane_wide[24x2112 / 24x4160 / 24x8192]
  lg_dout_border_kernel with 64 KB of dynamic LDS (H = 16384) test_wide_and_tall_frames_vs_oracle[16384x8 / 16384x16] (the launch)
  distances beyond chamfer_init_dist0 (H > 8192, W = 8192)   test_wide_and_tall_frames_vs_oracle[16384x8 ..., 24x8192, 8x8192]
  lg_ml_rows_kernel's s_pat[128] (W = 8192)                  test_ml_only_at_8192_columns_wide
  planes, top-k, gather, finish below one tile / word / window test_small_frames_vs_oracle, test_selection_with_a_model
  8192 tiles with W > 4096                                   test_large_frame_at_8192_tiles_wide
  make_plan's refusals                                       test_shapes_outside_the_limits_are_refused_wide
Every test that runs a wide or tall frame carries `wide` in its name: `-k wide` and `-k "not wide"` run the two groups apart."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import frame_shapes as FS  # noqa: E402
from tests import label_aware_ref as LR  # noqa: E402
from tests import ml_select_ref as MR  # noqa: E402
from tests import param_oracle as PO  # noqa: E402
from tests.test_gpu_grasp_candidates import _assert_rows_match_oracle, _by_index, _valid_rows  # noqa: E402
from tests.test_gpu_headline_batch import _assert_frame_equals_single  # noqa: E402
from tests.test_gpu_label_aware import dense_call  # noqa: E402
from tests.test_gpu_leaf_depths import _check_rows  # noqa: E402
from tests.test_gpu_params import _assert_triple, _call, _dev, _mask_tensor, _oracle_rows, _selector  # noqa: E402
from tests.test_gpu_parity import DT_FORMS, _compare_maps  # noqa: E402
from tests.test_gpu_sparse_planes import _assert_sparse_equals_dense  # noqa: E402
from tests.test_window_box_host import lib_window  # noqa: E402

FORCED = {"auto": 0, "search1": 1, "bands": 5, "sweep": 6}    # LG_DT_SEARCH_ALGO of each entry of DT_FORMS that searches
SEARCH_BUDGET = 2.0e7                                          # LG_SEARCH_BUDGET (lg_dt.h)
SMALL_ALL_FORMS = [(8, 8), (8, 9), (9, 8), (16, 16)]           # 16 x 16 and below: the forms differ (1 forced / 5 and 6 at sixteen)


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


# every small shape on the default handle; the shapes where the forms differ on a handle of each form as well
SMALL_RUNS = [(s, "auto") for s in FS.SMALL] + [(s, f) for s in SMALL_ALL_FORMS for f in DT_FORMS if f != "auto"]


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


@pytest.fixture(scope="module")
def form_sels(L):
    """one handle per entry of DT_FORMS, made under its switches (read when a handle is created), kept across the cases"""
    out = {}
    for name, env in DT_FORMS.items():
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            out[name] = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return out


@pytest.fixture(scope="module")
def cnn_sel(L):
    s = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    s.set_cnn_state_dict(PO.cnn_params())
    return s


def _apply(sel, params, P):
    sel.set_camera_params(P)
    for k, v in params.items():
        if k not in ("min_edge_distance", "gaussian_size", "mask_is_bool"):
            setattr(sel.params, k, v)
    sel.min_edge_distance = params["min_edge_distance"]


@functools.lru_cache(maxsize=None)
def _ip(H, W, g):
    import leafgrasp_amd

    return leafgrasp_amd.ImageProcessor(H, W, 21, g)


def _form_host(forced, H, W):
    from leafgrasp_amd import _lib

    return int(_lib.lib.lg_dt_form_host(forced, 1, H, W))


def _box_words(mask):
    xs = np.nonzero(mask.any(axis=0))[0]
    return (int(xs[-1]) >> 6) - (int(xs[0]) >> 6) + 1 if xs.size else 0


def _planes_and_candidates(sel, form, case, **changes):
    """tests/test_gpu_params.py::_planes_and_candidates on a Case and a kept handle, plus the two maxima of the distance
    transforms and the form that ran."""
    H, W = case.shape
    params = case.params(**changes)
    far = FS.far(H, W, params["chamfer_init_dist0"])
    mask, depth, P = case.scene()
    _apply(sel, params, P)
    ip = _ip(H, W, params["gaussian_size"])
    ref = PO.oracle(P, params)
    maps, valid, sc = _compare_maps(sel, mask, depth, P, ref=ref, image_processor=ip)
    what = f"{case.name} {form}"
    # ---- the maxima that normalise the sdf term, and the form
    mi, mo, win = sel.dt_maxima(0)
    d_in, d_out = sc["distance_map"], O.distance_transform(1 - mask, 5, init_dist0=params["chamfer_init_dist0"])
    assert mi == d_in.max(), (what, mi, d_in.max(), win)
    assert mo == d_out.max(), (what, mo, d_out.max(), win)
    searched, skipped_out = sel.dt_form(0)
    area = int(mask.sum())
    want = form != "sweeps" and 0 < area < H * W and not far    # a frame without a leaf or without a zero pixel is swept
    if want and form == "auto":                       # (lg_window_kernel: area^1.5 against the budget times the box's rows)
        rows = int(np.ptp(np.nonzero(mask.any(axis=1))[0])) + 1
        want = float(area) * float(np.sqrt(area)) <= SEARCH_BUDGET * rows
    assert searched == want, (what, searched, area)
    if form == "sweeps":
        assert sel.dt_search_form() == 0, what
    else:
        assert sel.dt_search_form() == _form_host(FORCED[form], H, W), what
    if area:   # d_out sweeps skipped: max d_out came from lg_dout_border_kernel alone (the window's own code, run on the host)
        ys, xs = np.nonzero(mask)
        box = np.array([W - 1 - xs.min(), xs.max(), H - 1 - ys.min(), ys.max(), area], np.uint32)
        assert skipped_out == (bool(lib_window(box, H, W, 1)[8]) and not far), what
        if case.kind == "corner" and max(H, W) >= 4096 and not far:
            assert skipped_out, what
    # ---- the candidates: the oracle's walk over the DEVICE's planes, then the pipeline's own rows against that
    k, md = params["top_k"], params["nms_min_distance"]
    got = sel._get_candidate_points(maps["traditional_score"], valid, k, md)
    wantc = ref._get_candidate_points(maps["traditional_score"].cpu().numpy(), valid.cpu().numpy().astype(bool), k, md)
    assert got == wantc and len(got) == case.n_cand, (what, got, wantc)
    _, cands = sel.select_grasp_candidates_batch(_mask_tensor(mask, params), _dev(depth), image_processor=ip, top_k=k)
    rows = _by_index(_valid_rows(cands[0]))
    assert [(int(r["x"]), int(r["y"])) for r in rows] == wantc, what
    return searched


# ----------------------------------------------------------------------------- planes, validity, theta, candidates
@pytest.mark.parametrize("shape,form", SMALL_RUNS, ids=[f"{_id(s)}-{f}" for s, f in SMALL_RUNS])
def test_small_frames_vs_oracle(form_sels, shape, form):
    """Every mask of a small shape: frames below one tile (H < 16), one 64-bit word with tail bits (W < 64), one word exactly,
    one pixel into the second word or tile row (65, 17).  On 16 x 16 and below every entry of DT_FORMS runs: below sixteen rows
    or columns forms 5 and 6 must fall back to 1, at exactly sixteen they run."""
    for case in FS.plane_cases(shape):
        _planes_and_candidates(form_sels[form], form, case)
    if form in ("bands", "sweep"):
        assert _form_host(FORCED[form], *shape) == (FORCED[form] if shape == (16, 16) else 1)


@pytest.mark.parametrize("form", list(DT_FORMS))
@pytest.mark.parametrize("shape", FS.WIDE_TALL, ids=_id)
def test_wide_and_tall_frames_vs_oracle(form_sels, shape, form):
    """W in (2048, 4096], (4096, 8192) and 8192, H = 16384.  `sweeps`: d_in and d_out by lg_dt5_kernel<512, 8> up to 4096
    columns and lg_dt5_kernel<1024, 8> above (no test had a frame wider than 3840).  The searching forms: lg_hrun_kernel on
    boxes wider than 64 words (band, ends and ellipse at 4160 and 8192 columns; `ends` leaves the middle words empty).
    H = 16384: lg_dout_border_kernel is launched with 4 * 16384 bytes of dynamic LDS (a refused launch would fail the call).
    Where a distance can reach chamfer_init_dist0 = 8192 px (FS.far: H = 16384, W = 8192) OpenCV's border cells cap the
    transform -- on the corner mask of 16384 x 8 max d_out is 8196, not 16376.6 -- and the library sweeps the whole frame;
    the W = 8192 frames run again under INT_MAX, where nothing is capped and the window, the border maxima and the row search
    (128-word rows) are back."""
    H, W = shape
    searched_wide = 0
    for case in FS.plane_cases(shape):
        s = _planes_and_candidates(form_sels[form], form, case)
        searched_wide += bool(s) and _box_words(case.scene()[0]) > 64
        if FS.far(H, W) and H < 16384:
            # the same frame under chamfer_init_dist0 = INT_MAX: no distance reaches it, the window and the row search are back
            s = _planes_and_candidates(form_sels[form], form, case, chamfer_init_dist0=FS.INT_MAX)
            searched_wide += bool(s) and _box_words(case.scene()[0]) > 64
    if form == "sweeps":
        assert FS.sweep_geometry(W) == ((1024, 8) if W > 4096 else (512, 8) if W > 2048 else (64, 4))
    elif W > 4096:
        # band and ends at 4160 columns (65 words; the ellipse spans 59), the ellipse too at 8192
        assert searched_wide >= 2, "the 64-word pieces of lg_hrun_kernel were not reached"


def test_large_frame_at_8192_tiles_wide(form_sels):
    """(1009, 8129): 64 x 128 tiles, the top-k tile table exactly full, W > 4096, odd W (no vector path), a last tile row of one
    pixel.  Planes, validity and candidates on the default handle; the one case above a few seconds (the oracle on 8 M pixels)."""
    H, W = FS.LARGE
    assert FS.tiles(H, W) == 8192
    (case,) = FS.plane_cases(FS.LARGE)
    assert FS.far(H, W) and not FS.far(H, W, FS.INT_MAX)
    assert not _planes_and_candidates(form_sels["auto"], "auto", case)                             # capped: swept whole
    assert _planes_and_candidates(form_sels["auto"], "auto", case, chamfer_init_dist0=FS.INT_MAX)   # window + row search


@pytest.mark.parametrize("case", FS.RUN_OUT, ids=lambda c: f"{c.name}-top{c.top_k}")
def test_small_frames_that_run_out_of_candidates(form_sels, case):
    """top_k = 20 or 64 on frames that cannot space that many: the device's walk ends where the oracle's does."""
    assert case.n_cand < case.top_k
    _planes_and_candidates(form_sels["auto"], "auto", case)


# ----------------------------------------------------------------------------- the whole selection with a model loaded
def _selection(cnn_sel, case, dtype):
    H, W = case.shape
    is_bool = int(dtype == "bool")
    params = case.params(mask_is_bool=is_bool)
    mask, depth, P = case.scene()
    exp = FS.run(case, True, is_bool)
    _apply(cnn_sel, params, P)
    ip = _ip(H, W, params["gaussian_size"])
    m, d = _mask_tensor(mask, params), _dev(depth)
    got = cnn_sel.select_grasp_point(m, d, ip)
    _assert_triple(got, exp["triple"])
    triples, cands = cnn_sel.select_grasp_candidates_batch(m, d, image_processor=ip, top_k=params["top_k"])
    _assert_triple(triples[0], exp["triple"])
    rows = _valid_rows(cands[0])
    _assert_rows_match_oracle(rows, _oracle_rows(exp, depth, mask), f"{case.name} {dtype}")
    assert (int(rows[0]["x"]), int(rows[0]["y"])) == exp["triple"][0]
    if not is_bool:
        assert rows["scored"].all()      # every 32 x 32 patch, replicated over whichever borders it crosses
    elif not FS.window_fits(H, W):
        assert not rows["scored"].any() and exp["triple"][0] == exp["candidates"][0]   # nothing scored: candidate 0


@pytest.mark.parametrize("dtype", ["uint8", "bool"])
@pytest.mark.parametrize("case", [c for c in FS.END_TO_END if c.shape in FS.SMALL], ids=lambda c: c.name)
def test_selection_with_a_model_small(cnn_sel, case, dtype):
    """Rows and triple against the oracle's own selection.  uint8: every candidate is scored, and on frames under 32 pixels a
    patch hangs over all four borders at once (lg_gather_kernel's replicate clamp in both directions).  bool: on frames under
    32 on a side no window fits, nothing may be scored and the pick is candidate 0."""
    _selection(cnn_sel, case, dtype)


@pytest.mark.parametrize("dtype", ["uint8", "bool"])
@pytest.mark.parametrize("case", [c for c in FS.END_TO_END if c.shape in FS.WIDE_TALL], ids=lambda c: c.name)
def test_selection_with_a_model_wide(cnn_sel, case, dtype):
    _selection(cnn_sel, case, dtype)


# ----------------------------------------------------------------------------- batches
def _three(shape):
    """leaf, empty, full of one shape"""
    e = FS.E2E_BY_SHAPE[shape]
    mask, depth, P = e.scene()
    masks = np.stack([mask, np.zeros_like(mask), np.ones_like(mask)]).astype(bool)
    return e, masks, np.stack([depth] * 3), P


def _batch_equals_single(L, shape):
    e, masks, depths, P = _three(shape)
    params = e.params()
    for with_cnn in (False, True):
        sel, ip = _selector(L, params, P, shape, with_cnn=with_cnn)
        maps, valid, triples, cands = _call(sel, ip, masks, depths, params["top_k"])
        for b in range(3):
            m1, v1, t1, c1 = _call(sel, ip, masks[b][None], depths[b][None], params["top_k"])
            for k in maps:
                assert maps[k][b].tobytes() == m1[k][0].tobytes(), (shape, k, b)
            assert valid[b].tobytes() == v1[0].tobytes(), (shape, b)
            rb, rs = _valid_rows(cands[b]), _valid_rows(c1[0])
            assert len(rb) == params["top_k"]
            if with_cnn:   # (the CNN's launch regime follows the patch count: its fields are held as the headline batch holds them)
                _assert_frame_equals_single(rb, rs, f"{shape} frame {b}")
            else:
                assert cands[b].tobytes() == c1[0].tobytes() and triples[b] == t1[0], (shape, b)
    sel.select_grasp_points_batch = functools.partial(sel.select_grasp_points_batch, image_processor=ip)
    tr = _assert_sparse_equals_dense(sel, masks, depths)
    assert tr[0][0] == FS.run(e, True)["triple"][0] and all(t[0] is not None for t in tr)


@pytest.mark.parametrize("shape", [(8, 9), (8, 65), (17, 65), (33, 31)], ids=_id)
def test_batch_of_three_equals_single_calls_small(L, shape):
    """leaf, empty and full frame of one shape in one call: planes, validity, rows and triples byte for byte those of the
    single calls, and the sparse call (no plane output) equals the dense one."""
    _batch_equals_single(L, shape)


@pytest.mark.parametrize("shape", [(24, 4160), (8, 8192), (16384, 8)], ids=_id)
def test_batch_of_three_equals_single_calls_wide(L, shape):
    _batch_equals_single(L, shape)


@pytest.mark.parametrize("order", [((8, 9), (24, 8192)), ((24, 8192), (8, 9)), ((16384, 16), (17, 65)), ((17, 65), (16384, 16))],
                         ids=lambda o: f"{_id(o[0])}-then-{_id(o[1])}")
def test_wide_and_small_on_one_handle_equal_fresh_handles(L, order):
    """A small case after a wide or tall one on the same handle, and the reverse: a workspace regrown (or kept too large, with
    strides of the earlier shape) would show in the planes, the validity or the rows."""
    used = None
    for shape in order:
        e, masks, depths, P = _three(shape)
        params = e.params()
        fresh, ip = _selector(L, params, P, shape, with_cnn=True)
        if used is None:
            used, _ = _selector(L, params, P, shape, with_cnn=True)
        _apply(used, params, P)
        a = _call(used, ip, masks, depths, params["top_k"])
        b = _call(fresh, ip, masks, depths, params["top_k"])
        for k in a[0]:
            assert a[0][k].tobytes() == b[0][k].tobytes(), (shape, k)
        assert a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes(), shape


# ----------------------------------------------------------------------------- label-aware selection
def _labels(H, W):
    """the current leaf (1), another leaf within 40 px of it (2), one at the far end of the frame (3)"""
    ry = max(2, int(0.4 * H))
    rx = min(30, max(4, W // 7))
    r2, gap, cx = max(2, rx // 2), min(12, max(3, W // 10)), rx + 1
    return LR.blob_labels(H, W, [(1, cx, H / 2.0, rx, ry), (2, cx + rx + gap + r2, H / 2.0, r2, ry), (3, W - 3, H / 2.0, 2, ry)])


@pytest.mark.parametrize("shape", [(8, 65), (31, 33), (24, 2112), (24, 4160), (24, 8192)], ids=_id)
def test_label_aware_fields_and_plane_wide(L, shape):
    """isolation_fields bit for bit and the isolation plane at the plane tolerance against tests/label_aware_ref.py.  W <= 2048
    runs lg_iso_sweep_kernel<8, *>, the three wide frames lg_iso_sweep_kernel<32, *> (65.5 KB of static LDS, 32 columns per
    thread), which no other test launches; (8, 65) and (31, 33): a frame of fewer rows than the 30 and 40 ellipses."""
    H, W = shape
    labels = _labels(H, W)
    cur, oth, _ = LR.split(labels, 1)
    xs1, xs2 = np.nonzero(cur.any(axis=0))[0], np.nonzero((labels == 2).any(axis=0))[0]
    assert 0 < xs2[0] - xs1[-1] < 40 and (labels == 3).any() and (labels == 3)[:, W - 8:].any()
    depth = FS.scene(H, W, "ellipse", 0)[1]
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_camera_params(FS.scene(H, W, "ellipse", 0)[2])
    planes0, valid0, _, _ = dense_call(L, sel, labels[None], [1], depth[None], False)
    planes1, valid1, _, _ = dense_call(L, sel, labels[None], [1], depth[None], True)
    got = sel.isolation_fields(0, H, W)
    assert got is not None, "the frame has other leaves: the transforms must have run"
    _, (dcf, dwf) = LR.transforms(oth)
    assert np.array_equal(got[0], dcf), ("dc", np.argwhere(got[0] != dcf)[:4])
    assert np.array_equal(got[1], dwf), ("dw", np.argwhere(got[1] != dwf)[:4])
    assert got[2] == (int(dcf.max()), int(dwf.max()))
    want = LR.isolation_plane(labels, 1)
    # (31, 33): the dilated neighbours cover the whole frame -- both fields and both maxima are 0, the plane is 0 on the leaf
    assert want.max() > 0 or shape == (31, 33)
    np.testing.assert_allclose(planes1["isolation_map"][0], want, rtol=1e-4, atol=1e-6)
    assert not np.array_equal(planes1["isolation_map"][0], planes0["isolation_map"][0]), "the plane must see the neighbour"
    for n in planes0:
        if n != "isolation_map":
            assert planes1[n].tobytes() == planes0[n].tobytes(), n
    assert valid1.tobytes() == valid0.tobytes()


# ----------------------------------------------------------------------------- ML-only selection
def _ml(L, mask, depth, P, mode, **kw):
    from leafgrasp_amd.grasp_point_selector import _RESULT_DTYPE

    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_cnn_state_dict(MR.params())
    sel.set_camera_params(P)
    s = sel.ml_sampling(mode, max_samples=4096, **kw)
    tri, rows, counts = sel.select_grasp_points_ml_batch(_dev(mask[None]), _dev(depth[None]), sampling=s, return_samples=True)
    res = np.frombuffer(bytes(sel.last_results), dtype=_RESULT_DTYPE)
    return tri[0], rows[0], int(counts[0]), res[0]


def _ml_against_ref(L, H, W, mask, mode, **kw):
    """the sample table bit for bit, the scored samples' logits at the CNN tolerance, the pick or the centroid fall-back"""
    _, depth, P = FS.scene(H, W, "full", 0)
    n, xy, scored, sums = MR.table(mask, MR.NTH if mode == "nth" else MR.GRID, **kw)
    tri, rows, count, res = _ml(L, mask, depth, P, mode, **kw)
    assert count == n >= 0      # (8 x 8, stride 8: the ellipse misses the one grid pixel (0, 0): no sample at all)
    assert np.array_equal(rows["x"][:n], xy[:, 0]) and np.array_equal(rows["y"][:n], xy[:, 1])
    assert np.array_equal(rows["scored"][:n], scored)
    assert not rows[n:].tobytes().strip(b"\0")
    ref = MR.ref_selector(P)
    m8 = np.ascontiguousarray(mask, np.uint8)
    if scored.any():
        logits = MR.oracle_logits(ref, mask, depth, xy, scored)
        sc = scored == 1
        assert np.abs(rows["logit"][:n][sc].astype(np.float64) - logits[sc]).max() <= 1e-4
        pick = MR.first_max(np.where(sc, rows["logit"][:n].astype(np.float64), np.nan))
        if MR.margin(logits) > 2e-4:
            assert pick == MR.first_max(logits)
        pt = (int(xy[pick, 0]), int(xy[pick, 1]))
        assert res["ml_used"] == 1
    else:
        pt = MR.centroid(sums)
        assert res["ml_used"] == 0 and np.isnan(res["best_score"])
    assert tri[0] == pt and res["found"] == 1 and res["n_candidates"] == int(scored.sum())
    g3 = ref.get_3d_grasp_point(pt, depth)
    np.testing.assert_allclose(tri[1], g3, rtol=1e-5)
    np.testing.assert_allclose(tri[2], ref.calculate_pre_grasp_point(g3, m8), rtol=1e-5)
    return scored, xy


@pytest.mark.parametrize("mode,kw", [("nth", dict(target=100)), ("grid", dict(stride=8)), ("grid", dict(stride=1))],
                         ids=["nth", "grid8", "grid1"])
@pytest.mark.parametrize("shape", [(8, 8), (31, 40), (33, 33)], ids=_id)
def test_ml_only_on_small_frames(L, shape, mode, kw):
    """Frames around one CNN window: at 8 x 8 and 31 x 40 no sample lies off the 16-pixel border band (the centroid fall-back),
    at 33 x 33 exactly the pixel (16, 16) does (reference :326-328: y < 16 or y >= H - 16 is skipped), which grid sampling
    reaches and every-10th-pixel sampling does not."""
    H, W = shape
    mask = FS.mask_of(H, W, "full" if shape == (33, 33) else "ellipse")
    scored, xy = _ml_against_ref(L, H, W, mask, mode, **kw)
    if shape == (33, 33) and mode == "grid":
        assert scored.sum() == 1 and tuple(xy[scored == 1][0]) == (16, 16)
    else:
        assert not scored.any()


@pytest.mark.parametrize("mode,kw", [("nth", dict(target=100)), ("grid", dict(stride=8))], ids=["nth", "grid8"])
def test_ml_only_at_8192_columns_wide(L, mode, kw):
    """lg_ml_rows_kernel holds one sampling pattern per word in s_pat[128]: W = 8192 fills it.  The band mask has samples in
    the last word; the table must be NumPy's to the bit (H = 24 < 32: nothing is scored, the centroid is returned)."""
    H, W = 24, 8192
    mask = FS.mask_of(H, W, "band")
    scored, xy = _ml_against_ref(L, H, W, mask, mode, **kw)
    assert FS.words(W) == 128 and (xy[:, 0] >= W - 64).any() and not scored.any()


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("shape", FS.REFUSED_SHAPES, ids=_id)
def test_shapes_outside_the_limits_are_refused_wide(L, cnn_sel, shape):
    """make_plan: H < 8, W < 8, W > 8192, H > 16384 are LG_ERR_INVALID (-1), more than 8192 tiles LG_ERR_UNSUPPORTED (-5),
    from every entry that plans a call.  The device inputs have the refused shape's own size, so a missing guard could not
    read or write outside them.  Afterwards the same handle answers a normal call."""
    H, W = shape
    status = "status -5" if FS.tiles(H, W) > 8192 and 8 <= H <= 16384 and 8 <= W <= 8192 else "status -1"
    e = FS.E2E_BY_SHAPE[(17, 65)]
    _apply(cnn_sel, e.params(), e.scene()[2])
    m, d = torch.zeros((1, H, W), dtype=torch.bool, device="cuda"), torch.full((1, H, W), 0.5, device="cuda")
    m[:, 2:6, 2:6] = True
    for call in (lambda: cnn_sel.score_maps(m, d), lambda: cnn_sel.select_grasp_points_batch(m, d),
                 lambda: cnn_sel.select_grasp_candidates_batch(m, d, top_k=4), lambda: cnn_sel.select_grasp_points_ml_batch(m, d)):
        with pytest.raises(L.LgError, match=status):
            call()
    assert cnn_sel.select_grasp_point(m[0], d[0], None) == (None, None, None)   # through the mirror: the None triple
    del m, d
    _selection(cnn_sel, e, "uint8")


def test_init_dist0_above_the_default_is_refused_at_16384_rows_wide(L, cnn_sel):
    """The sweeps mark "no path" with 16384.0 in 16.16: a real distance has to stay below it unless OpenCV's border cells hide
    it, which they do up to chamfer_init_dist0 = INT_MAX >> 2.  make_plan refuses the rest (LG_ERR_UNSUPPORTED): a larger
    chamfer_init_dist0 on a frame whose diagonal reaches 16384 px.  16376 rows under INT_MAX are served."""
    e = FS.E2E_BY_SHAPE[(16384, 8)]
    mask, depth, P = e.scene()
    _apply(cnn_sel, e.params(chamfer_init_dist0=FS.INT_MAX), P)
    ip = _ip(16384, 8, 3)
    with pytest.raises(L.LgError, match="status -5"):
        cnn_sel.score_maps(_dev(mask), _dev(depth), ip)
    case = FS.Case(16376, 8, "corner", 0)
    assert FS.norm5(7, 16375) + 2 * 143976 < 0x3FFFFFFF and not FS.far(16376, 8, FS.INT_MAX)
    _planes_and_candidates(cnn_sel, "auto", case, chamfer_init_dist0=FS.INT_MAX)   # max d_out = 16368.6 from the border line alone
    _selection(cnn_sel, e, "uint8")


# ----------------------------------------------------------------------------- leaf statistics at their width limit
def test_leaf_stats_accepts_4096_columns_and_refuses_4097_wide(L):
    """lg_leaf_stats: W = 4096 is its widest frame (areas, coordinate sums, medians and depth sums against NumPy, as
    tests/test_gpu_leaf_depths.py compares); 4097 is refused with its message."""
    H, W = 24, 4096
    labels = LR.blob_labels(H, W, [(1, 40, 12, 30, 9), (2, 2000, 12, 300, 10), (3, W - 20, 12, 19, 11), (4, 3000, 4, 90, 3)])
    assert (labels[:, W - 1] == 3).any() and (labels[:, 0] == 0).all()
    depth = FS.scene(H, W, "full", 0)[1]
    ols = L.OptimalLeafSelector("cuda:0")
    ols.set_camera_params(FS.scene(H, W, "full", 0)[2])
    rows = ols.leaf_statistics(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda())[0]
    assert len(rows) == 4
    _check_rows(rows, labels, depth, tag="24x4096")
    wide = np.zeros((H, W + 1), np.int16)
    wide[:, :W] = labels
    with pytest.raises(L.LgError, match="width > 4096 unsupported"):
        ols.leaf_statistics(torch.from_numpy(wide).cuda(), torch.from_numpy(np.full((H, W + 1), 0.5, np.float32)).cuda())
    _check_rows(ols.leaf_statistics(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda())[0], labels, depth, tag="again")
