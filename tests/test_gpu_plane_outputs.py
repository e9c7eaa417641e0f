"""The plane kernel under every subset of outputs include/leafgrasp.h allows: out_maps[i] "any entry may be NULL = not wanted",
out_valid "may be NULL" -- 2^8 x 2 combinations per entry, of which the rest of the suite asks for two (everything, nothing).
The calls go through ctypes on a GraspPointSelector's handle; cases and subsets: tests/plane_outputs.py; their premises (valid
pixels, no near-tie, the tile classes of the two frames): tests/test_plane_outputs_host.py.

Which lg_final_kernel<VEC, ALL, R, SCORE> a call reaches is a pure function of (W % 4, gaussian_size, the NULL pointers, the
entry, a loaded model) -- lg_select.hip take_planes, lg_planes.hip lg_launch_final; plane_outputs.store_form restates it:
  VEC    = W % 4 == 0                                     264 / 263
  R      = gaussian_size / 2                              0, 1, 2, 3
  SCORE  = lg_select_grasp* with no plane and no validity (sparse mode, deferred planes)
  ALL    = not SCORE and no pointer left NULL after take_planes, which fills in workspace planes for DISTANCE and TRADITIONAL
           always, for all eight when a model is loaded (a non-sparse lg_select_grasp*), and the workspace validity plane:
           every plane but possibly DISTANCE / TRADITIONAL given, with or without validity; or any subset beside a model
  neither (the partial form, <VEC, false, R>): every other call -- some plane other than DISTANCE / TRADITIONAL is NULL and
           no model stands behind a select call.  2 x 4 instantiations that no other test launches:
    <true,  false, 2> / <false, false, 2>   test_score_maps_every_subset[264 / 263], test_select_grasp_named_subsets[*-no model]
    <true,  false, 0 / 1 / 3>               test_score_maps_named_subsets[264-*-g1 / g3 / g7], test_select_grasp_other_radii[264-*]
    <false, false, 0 / 1 / 3>               test_score_maps_named_subsets[263-*-g1 / g3 / g7], test_select_grasp_other_radii[263-*]
The partial form squares the gradient with the other product fused (lg_flat4<VEC && (ALL || SCORE)>, lg_pixel.h):
its flatness and traditional planes may differ from a full call's in the last bit, by design.  Nothing here compares floats
between subsets; every call is held to the oracle at the project's tolerances, and the rows to the same grasp pixel.

Every plane, passed or not, lies in a buffer with a guard band of 16 rows in front and behind (16: the planes keep the 16-byte
alignment a frame of a batch has), prefilled with NaN (validity: 0xA5): a pixel the kernel left unwritten, a write outside a
plane and a write to a plane that was not passed all show.  Tolerances: distance_map, stem_penalty and validity bit for bit,
the float planes rtol 1e-4 / atol 1e-6 (tests/test_gpu_parity.py), triples rtol 1e-5."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import label_aware_ref as LR  # noqa: E402
from tests import param_oracle as PO  # noqa: E402
from tests import plane_outputs as PL  # noqa: E402
from tests.test_gpu_parity import ATOL, RTOL  # noqa: E402

G = 16            # guard rows
H = PL.H
NAN = float("nan")
PARTIAL3 = [("validity alone", frozenset(), True), ("flatness_map alone", frozenset([PL.FLATNESS]), False),
            ("all but flatness_map", PL.ALL - {PL.FLATNESS}, True)]


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


def _new(L, model=False, env=None):
    """a selector (its handle is what the calls below use); `env`: switches lg_create reads, set and restored around it"""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if model:
        sel.set_cnn_state_dict(PO.cnn_params())
    return sel


@pytest.fixture(scope="module")
def plain(L):
    return _new(L)


@pytest.fixture(scope="module")
def with_model(L):
    return _new(L, model=True)


def _lg_params(params, P):
    from leafgrasp_amd import _lib

    p = _lib.default_params()
    p.cx, p.cy, p.f = float(P[0, 2]), float(P[1, 2]), float(P[0, 0])
    for k, v in params.items():
        setattr(p, k, v)
    return p


# ----------------------------------------------------------------------------- buffers and expectations
class Buffers:
    """eight planes and a validity plane for B frames of H x W, each between two guard bands"""

    def __init__(self, B, W):
        self.B, self.W = B, W
        rows = B * H + 2 * G
        self.maps = torch.empty((8, rows, W), dtype=torch.float32, device="cuda")
        self.valid = torch.empty((rows, W), dtype=torch.uint8, device="cuda")
        assert all(self.maps[i, G].data_ptr() % 16 == 0 for i in range(8)) and self.valid[G].data_ptr() % 16 == 0

    def prefill(self):
        self.maps.fill_(NAN)
        self.valid.fill_(0xA5)

    def pointers(self, planes, valid):
        from leafgrasp_amd._lib import LG_NUM_MAPS

        ptrs = (C.c_void_p * LG_NUM_MAPS)()
        for i in range(LG_NUM_MAPS):
            ptrs[i] = self.maps[i, G].data_ptr() if i in planes else None
        return ptrs, (self.valid[G].data_ptr() if valid else None)

    def body(self):
        return self.maps[:, G:G + self.B * H].view(8, self.B, H, self.W)

    def vbody(self):
        return self.valid[G:G + self.B * H].view(self.B, H, self.W)

    def guards_touched(self):
        m = (~torch.isnan(self.maps[:, :G])).sum() + (~torch.isnan(self.maps[:, G + self.B * H:])).sum()
        return m + (self.valid[:G] != 0xA5).sum() + (self.valid[G + self.B * H:] != 0xA5).sum()


@functools.lru_cache(maxsize=None)
def _buffers(B, W):
    return Buffers(B, W)


class Want:
    """the oracle's planes and validity of a batch on the device, computed once"""

    def __init__(self, runs):
        sc = np.stack([np.stack([np.asarray(r["scores"][k], np.float64) for r in runs]) for k in PL.PLANES])
        self.planes = torch.from_numpy(sc).cuda()                                                        # [8, B, H, W] float64
        self.valid = torch.from_numpy(np.stack([r["valid"] for r in runs]).astype(np.uint8)).cuda()
        rt = torch.tensor([0.0 if i in PL.EXACT else RTOL for i in range(8)], dtype=torch.float64).view(8, 1, 1, 1)
        at = torch.tensor([0.0 if i in PL.EXACT else ATOL for i in range(8)], dtype=torch.float64).view(8, 1, 1, 1)
        self.tol = (at + rt * torch.from_numpy(np.abs(sc))).cuda()    # np.testing.assert_allclose: |got - want| <= atol + rtol |want|
        self.runs = runs


@functools.lru_cache(maxsize=None)
def _want(W, name, g, seeds=None, with_cnn=False, default_params=False):
    seeds = seeds or (None,)
    return Want([PL.run(W, name, g, s, with_cnn, default_params) for s in seeds])


@functools.lru_cache(maxsize=None)
def _inputs(W, name, seeds):
    sc = [PL.scene(W, name, s) for s in seeds]
    mask = torch.from_numpy(np.stack([s[0] for s in sc])).cuda()
    depth = torch.from_numpy(np.stack([s[1] for s in sc])).cuda()
    return mask, depth, sc[0][2]


def _check_buffers(buf, want, planes, valid, what):
    """every plane passed equals the oracle, every guard band and every buffer not passed is untouched"""
    got = buf.body()
    passed = torch.tensor([i in planes for i in range(8)], device="cuda").view(8, 1, 1, 1)
    off = ~((got.double() - want.planes).abs() <= want.tol)        # (a NaN left in a passed plane is off)
    bad = torch.where(passed, off, ~torch.isnan(got))
    vbad = (buf.vbody() != want.valid) if valid else (buf.vbody() != 0xA5)
    n = int((bad.sum() + vbad.sum() + buf.guards_touched()).item())
    if n == 0:
        return
    g, w = got.cpu().numpy(), want.planes.cpu().numpy()
    lines = []
    for i in range(8):
        b = bad[i].cpu().numpy()
        if b.any():
            at = tuple(int(v) for v in np.argwhere(b)[0])
            lines.append(f"{PL.PLANES[i]} ({'passed' if i in planes else 'not passed'}): {int(b.sum())} pixels, first (frame, y, x) "
                         f"{at}: got {float(g[i][at])!r} want {float(w[i][at])!r}")
    if bool(vbad.any()):
        at = tuple(int(v) for v in np.argwhere(vbad.cpu().numpy())[0])
        lines.append(f"validity ({'passed' if valid else 'not passed'}): {int(vbad.sum())} pixels, first {at}: "
                     f"got {int(buf.vbody()[at])} want {int(want.valid[at]) if valid else 0xA5}")
    lines.append(f"guard bands: {int(buf.guards_touched())} elements touched")
    raise AssertionError(f"{what}, subset {PL.subset_id(planes, valid)}:\n  " + "\n  ".join(lines))


def _check_theta(theta, runs, what):
    for t, r in zip(theta, runs):
        assert r["theta"] is not None and abs(float(t) - r["theta"]) <= 1e-6, (what, float(t), r["theta"])


def _score_maps(sel, W, name, g, planes, valid, seeds=None, theta=True, null_params=False):
    from leafgrasp_amd import _lib

    seeds = seeds or (PL.SEEDS[(W, g)],)
    B = len(seeds)
    mask, depth, P = _inputs(W, name, seeds)
    want = _want(W, name, g, seeds, False, null_params)
    buf = _buffers(B, W)
    buf.prefill()
    ptrs, vptr = buf.pointers(planes, valid)
    p = _lg_params(PL.params_of(W, g), P)
    th = (C.c_float * B)(*([NAN] * B))
    rc = _lib.lib.lg_score_maps(sel._h, depth.data_ptr(), mask.data_ptr(), B, H, W, None if null_params else C.byref(p), C.byref(ptrs),
                                vptr, th if theta else None, sel._stream())
    what = f"lg_score_maps {W} {name} g={g} B={B}"
    assert rc == _lib.LG_OK, (what, PL.subset_id(planes, valid), _lib.lib.lg_last_error(sel._h))
    _check_buffers(buf, want, planes, valid, what)
    if theta:
        _check_theta(th, want.runs, what)
    else:
        assert all(np.isnan(t) for t in th)


# ----------------------------------------------------------------------------- lg_score_maps
@pytest.mark.parametrize("W", PL.WIDTHS)
def test_score_maps_every_subset(plain, W):
    """All 512 (plane subset, validity given or not) on `interior` at gaussian_size 5, one handle: 504 calls of
    lg_final_kernel<W % 4 == 0, false, 2>, 8 of <.., true, 2> between them."""
    forms = set()
    for planes, valid in PL.EXHAUSTIVE:
        _score_maps(plain, W, "interior", 5, planes, valid)
        forms.add(PL.instantiation(W, 5, planes, valid))
    assert forms == {(W % 4 == 0, False, 2, False), (W % 4 == 0, True, 2, False)}


@pytest.mark.parametrize("g", [1, 3, 7])
@pytest.mark.parametrize("name", PL.SCENES)
@pytest.mark.parametrize("W", PL.WIDTHS)
def test_score_maps_named_subsets(plain, W, name, g):
    """The named subsets at the other three radii, on both scenes: `corner` puts the reflect staging (top and left frame edge)
    and the partial last tile column on the stencil path of the partial form."""
    forms = set()
    for _, planes, valid in PL.NAMED:
        _score_maps(plain, W, name, g, planes, valid)
        forms.add(PL.instantiation(W, g, planes, valid))
    assert (W % 4 == 0, False, g // 2, False) in forms


@pytest.mark.parametrize("W", PL.WIDTHS)
def test_score_maps_without_theta_and_without_params(plain, W):
    """theta_host = NULL: the planes as ever, nothing written through the pointer.  p = NULL: lg_default_params, i.e. the
    reference's constants with the camera at 707 / 494 and f unset (0: the approach plane is zero)."""
    for _, planes, valid in PARTIAL3 + [("full", *PL.FULL)]:
        _score_maps(plain, W, "interior", 5, planes, valid, theta=False)
        _score_maps(plain, W, "interior", 5, planes, valid, null_params=True)
    assert not _want(W, "interior", 5, None, False, True).runs[0]["scores"]["approach_score"].any()


@pytest.mark.parametrize("W", PL.WIDTHS)
def test_score_maps_batch_of_three(L, W):
    """Three frames with three seeds: a frame offset applied to a workspace plane and not to a caller's plane, or the reverse,
    puts one frame's pixels into another's place."""
    sel = _new(L)
    for _, planes, valid in PL.NAMED:
        _score_maps(sel, W, "interior", 5, planes, valid, seeds=(0, 1, 2))


# ----------------------------------------------------------------------------- lg_select_grasp
def _oracle_row(r):
    """the reference's selection loop (:205-236) over the oracle's candidates: pick, best_score, ml_used"""
    cands = r["candidates"]
    trad = [float(r["scores"]["traditional_score"][y, x]) for x, y in cands]
    best, best_score, ml_used = 0, trad[0], 0
    for i, m in enumerate(r["ml_scores"] or []):
        if m is not None:
            w = min(0.3, (1.0 - abs(m - 0.5) * 2) * 0.6)
            comb = (1.0 - w) * trad[i] + w * m
            if comb > best_score:
                best, best_score, ml_used = i, comb, 1
    assert cands[best] == r["triple"][0]
    return dict(xy=cands[best], best_score=best_score, ml_used=ml_used, n=len(cands), g3=r["triple"][1], pre=r["triple"][2],
                theta=r["theta"])


def _check_row(row, r, what):
    """found, grasp pixel, n_candidates, ml_used, best_score, 3-D point, pre-grasp point, theta against the oracle"""
    o = _oracle_row(r)
    assert row.found == 1 and (row.x, row.y) == o["xy"], (what, (row.x, row.y), o["xy"])
    assert row.n_candidates == o["n"] and row.ml_used == o["ml_used"], (what, row.n_candidates, row.ml_used, o)
    if o["ml_used"]:    # a combined score: the tolerance of the ML fields (tests/test_gpu_grasp_candidates.py)
        assert abs(row.best_score - o["best_score"]) <= 1e-4, (what, row.best_score, o["best_score"])
    else:
        np.testing.assert_allclose(row.best_score, o["best_score"], rtol=RTOL, atol=ATOL, err_msg=what)
    np.testing.assert_allclose([row.X, row.Y, row.Z], o["g3"], rtol=1e-5, err_msg=what)
    assert bool(row.has_pre) == (o["pre"] is not None), what
    if o["pre"] is not None:
        np.testing.assert_allclose([row.pX, row.pY, row.pZ], o["pre"], rtol=1e-5, err_msg=what)
    assert abs(row.theta - o["theta"]) <= 1e-6, what


def _select(sel, model, W, g, planes, valid, seeds=None, check_rows=True):
    """lg_select_grasp on `interior`; out_maps = out_valid = NULL for the empty subset (sparse mode).  Returns the rows."""
    from leafgrasp_amd import _lib

    seeds = seeds or (PL.SEEDS[(W, g)],)
    B = len(seeds)
    mask, depth, P = _inputs(W, "interior", seeds)
    want = _want(W, "interior", g, seeds, model)
    buf = _buffers(B, W)
    buf.prefill()
    ptrs, vptr = buf.pointers(planes, valid)
    sparse = not planes and not valid
    p = _lg_params(PL.params_of(W, g), P)
    res = (_lib.LgGraspResult * B)()
    rc = _lib.lib.lg_select_grasp(sel._h, depth.data_ptr(), mask.data_ptr(), B, H, W, C.byref(p), None if sparse else C.byref(ptrs),
                                  vptr, res, sel._stream())
    what = f"lg_select_grasp {W} g={g} B={B} model={model} subset {PL.subset_id(planes, valid)}"
    assert rc == _lib.LG_OK, (what, _lib.lib.lg_last_error(sel._h))
    _check_buffers(buf, want, planes, valid, what)
    if check_rows:
        for b in range(B):
            _check_row(res[b], want.runs[b], f"{what} frame {b}")
    return res


def _same_pixels(res, res0, what):
    for a, b in zip(res, res0):
        assert (a.found, a.x, a.y, a.n_candidates) == (b.found, b.x, b.y, b.n_candidates), what


@pytest.mark.parametrize("model", [False, True], ids=["no model", "model"])
@pytest.mark.parametrize("W", PL.WIDTHS)
def test_select_grasp_named_subsets(plain, with_model, W, model):
    """The named subsets behind top-k, the gather and the finish: without a model the partial form's own planes feed the
    candidates; with the closed-form model take_planes mixes the caller's planes with workspace planes for all the others and
    the gather reads both.  Planes, row against the oracle, the same grasp pixel as the call that takes nothing back."""
    sel = with_model if model else plain
    res0 = _select(sel, model, W, 5, *PL.NOTHING)
    for name, planes, valid in PL.NAMED:
        _same_pixels(_select(sel, model, W, 5, planes, valid), res0, name)
    _same_pixels(_select(sel, model, W, 5, *PL.FULL), res0, "full")
    assert PL.store_form(frozenset(), True, "select", model) == ("all" if model else "partial")


@pytest.mark.parametrize("g", [1, 3, 7])
@pytest.mark.parametrize("W", PL.WIDTHS)
def test_select_grasp_other_radii(plain, with_model, W, g):
    for model, sel in ((False, plain), (True, with_model)):
        res0 = _select(sel, model, W, g, *PL.NOTHING)
        for name, planes, valid in PARTIAL3:
            _same_pixels(_select(sel, model, W, g, planes, valid), res0, name)


@pytest.mark.parametrize("model", [False, True], ids=["no model", "model"])
def test_one_handle_across_forms_and_widths(L, model):
    """Full, partial and sparse calls alternate on one handle, at both widths (a change of width regrows the workspace) and two
    radii: a workspace plane left over from the previous call must not stand in for a store the current call owes.  Every
    call's planes and rows are held to the oracle like a first call's."""
    sel = _new(L, model=model)
    part = {n: (p, v) for n, p, v in PL.NAMED}
    order = [("maps", 264, 5, PL.FULL), ("select", 264, 5, part["validity alone"]), ("select", 264, 5, PL.NOTHING),
             ("maps", 264, 5, part["flatness_map alone"]), ("select", 263, 5, PL.NOTHING), ("maps", 263, 5, part["all but sdf_score"]),
             ("select", 263, 5, PL.FULL), ("select", 263, 3, part["traditional_score alone"]), ("select", 263, 3, PL.NOTHING),
             ("maps", 263, 3, part["validity alone"]), ("select", 264, 3, part["distance and traditional alone"]),
             ("maps", 264, 3, PL.FULL), ("select", 264, 3, part["all but stem_penalty"]), ("select", 264, 5, PL.NOTHING),
             ("maps", 264, 5, part["all but distance and traditional"]), ("select", 264, 5, part["isolation_map alone"])]
    pixels = {}
    for entry, W, g, (planes, valid) in order:
        if entry == "maps":
            _score_maps(sel, W, "interior", g, planes, valid)
        else:
            r = _select(sel, model, W, g, planes, valid)[0]
            assert pixels.setdefault((W, g), (r.x, r.y)) == (r.x, r.y)


def test_subbatch_pipeline(L):
    """LG_SUBBATCH=2 (read by lg_create): five frames run as three sub-batches on the handle's own streams, every stage with
    its frame offset into the caller's planes and the workspace planes alike.  Planes against the oracle; the rows equal those
    of a handle with one sub-batch (grasp pixel, counts; floats at the triple tolerance), and the oracle's on the frames of
    the seed that has no near-tie."""
    seeds = (1, 0, 1, 2, 1)
    assert PL.SEEDS[(264, 5)] == PL.SEEDS[(263, 5)] == 1
    by_name = {n: (n, p, v) for n, p, v in PL.NAMED}
    # without a model the partial form writes five of the caller's planes; with one, validity comes back beside eight workspace planes
    for model, (name, planes, valid) in ((False, by_name["all but flatness_map"]), (True, by_name["validity alone"])):
        piped, one = _new(L, model, {"LG_SUBBATCH": "2"}), _new(L, model)
        assert piped.options()["LG_SUBBATCH"] == 2 and one.options()["LG_SUBBATCH"] == 0
        for W in PL.WIDTHS:
            a = _select(piped, model, W, 5, planes, valid, seeds, check_rows=False)
            b = _select(one, model, W, 5, planes, valid, seeds, check_rows=False)
            want = _want(W, "interior", 5, seeds, model)
            for i, (ra, rb) in enumerate(zip(a, b)):
                what = f"LG_SUBBATCH=2 {W} {name} frame {i}"
                assert (ra.found, ra.x, ra.y, ra.n_candidates, ra.ml_used, ra.has_pre) == \
                       (rb.found, rb.x, rb.y, rb.n_candidates, rb.ml_used, rb.has_pre), what
                np.testing.assert_allclose([ra.X, ra.Y, ra.Z, ra.pX, ra.pY, ra.pZ], [rb.X, rb.Y, rb.Z, rb.pX, rb.pY, rb.pZ],
                                           rtol=1e-5, err_msg=what)
                assert abs(ra.best_score - rb.best_score) <= 1e-4, what
                if seeds[i] == 1:
                    _check_row(ra, want.runs[i], what)


# ----------------------------------------------------------------------------- lg_select_grasp_labels, label_aware = 1
def test_label_aware_subsets(L):
    """Two leaves 12 px apart (tests/test_gpu_label_aware.py, "nearer than 15 px"), the model loaded: the isolation plane is
    written by lg_iso_plane_kernel behind the plane kernel, into the caller's plane or into the workspace plane take_planes
    chose.  Subsets with and without ISOLATION: every plane passed against LabelAwareRef (the isolation plane:
    LR.isolation_plane), the row the full call's grasp pixel."""
    from leafgrasp_amd import _lib
    from tests.test_gpu_label_aware import P_of, cnn_params, depth_of

    Hl, Wl = 96, 128
    labels = LR.blob_labels(Hl, Wl, [(1, 50, 48, 26, 24), (2, 88, 48, 6, 8)])
    depth, P = depth_of(Hl, Wl), P_of(600.0, Wl / 2.0, Hl / 2.0)
    ref = LR.LabelAwareRef(labels, 1)
    ref.set_camera_params(P)
    sc = ref._calculate_all_scores(ref.current, depth)
    assert np.array_equal(sc["isolation_map"], LR.isolation_plane(labels, 1)) and sc["isolation_map"].max() > 0
    want = Want([dict(scores=sc, valid=ref._get_valid_regions(ref.current, sc))])
    assert int(want.valid.sum()) >= 8
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_cnn_state_dict(cnn_params())
    lab, d = torch.from_numpy(labels[None]).cuda(), torch.from_numpy(depth[None]).cuda()
    p = _lib.default_params()
    p.cx, p.cy, p.f = float(P[0, 2]), float(P[1, 2]), float(P[0, 0])
    p.label_aware = 1
    ids = (C.c_int32 * 1)(1)

    class Buf(Buffers):
        def __init__(self):
            self.B, self.W = 1, Wl
            self.maps = torch.empty((8, Hl + 2 * G, Wl), dtype=torch.float32, device="cuda")
            self.valid = torch.empty((Hl + 2 * G, Wl), dtype=torch.uint8, device="cuda")

        def body(self):
            return self.maps[:, G:G + Hl].view(8, 1, Hl, Wl)

        def vbody(self):
            return self.valid[G:G + Hl].view(1, Hl, Wl)

        def guards_touched(self):
            m = (~torch.isnan(self.maps[:, :G])).sum() + (~torch.isnan(self.maps[:, G + Hl:])).sum()
            return m + (self.valid[:G] != 0xA5).sum() + (self.valid[G + Hl:] != 0xA5).sum()

    buf = Buf()
    subsets = [("full", *PL.FULL), ("isolation alone", frozenset([PL.ISOLATION]), False), ("all but isolation", PL.ALL - {PL.ISOLATION}, True),
               ("isolation and validity", frozenset([PL.ISOLATION]), True), ("validity alone", frozenset(), True),
               ("sdf and flatness", frozenset([PL.SDF, PL.FLATNESS]), False), ("all but distance and traditional", PL.ALL - {PL.DISTANCE, PL.TRADITIONAL}, True)]
    pixel = None
    for name, planes, valid in subsets:
        buf.prefill()
        ptrs, vptr = buf.pointers(planes, valid)
        res = (_lib.LgGraspResult * 1)()
        rc = _lib.lib.lg_select_grasp_labels(sel._h, d.data_ptr(), lab.data_ptr(), ids, 1, Hl, Wl, C.byref(p), C.byref(ptrs), vptr, res,
                                             sel._stream())
        assert rc == _lib.LG_OK, (name, _lib.lib.lg_last_error(sel._h))
        _check_buffers(buf, want, planes, valid, f"lg_select_grasp_labels {name}")
        assert res[0].found == 1
        pixel = pixel or (res[0].x, res[0].y)
        assert (res[0].x, res[0].y) == pixel, name
    assert ref.current[pixel[1], pixel[0]]
