"""Label-aware mode (lg_params.label_aware = 1) on the device, against tests/label_aware_ref.py:

  transforms, plane   lg_debug_isolation_fields equals the oracle's fixed-point 3x3 transforms of the dilated other leaves bit for
                      bit, both whole-frame maxima included; the isolation plane of the dense call is within 1e-4 relative of
                      the reference (the tolerance of the float planes everywhere in this suite: float32 against the reference's
                      float64 ramp), every other plane and the validity plane keep the bytes of the label_aware = 0 call.
                      Neighbours nearer than 15 px, between 15 and 20 px, beyond 20 px, on every frame edge with the current leaf
                      on an edge, others covering everything but the leaf (maxima 0, plane 0), negative labels, an absent leaf
                      id (found = 0 from the Python entry's None; the C entry's fall-through picks are those of the flag off);
                      W % 64 == 0, W % 16 != 0 (the pack fall-back), and a frame of several tile rows.
  empty others        planes, rows and candidates equal the label_aware = 0 call bit for bit.
  pre-grasp           a neighbour on the camera ray: the default call's point lies on it (or within its clearance), the
                      label-aware call gives the reference's next clear step or the 0.10 m fall-back; every ranked candidate too.
  CNN channel         channel 5 of the patches (sparse / deferred and dense) equals the reference's normalised window at 1e-4,
                      the logits oracle.cnn_forward of the reference patches at 1e-4.
  batches             mixed batches of 3 and 5 frames equal the frames one at a time, bit for bit.
  default path        label_aware = 0 after a label-aware call on the same handle gives what it gave before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_aware_ref as R  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402

K = 20


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


def P_of(f, cx, cy):
    P = np.zeros((3, 4))
    P[0, 0] = P[1, 1] = f
    P[0, 2], P[1, 2], P[0, 3] = cx, cy, -0.1 * f
    return P


def depth_of(H, W, z=0.45):
    yy, xx = np.mgrid[:H, :W]
    return (z + 0.002 * np.sin(xx / 7.0) + 0.002 * np.cos(yy / 5.0)).astype(np.float32)


CNN = None


def cnn_params():
    global CNN
    if CNN is None:
        CNN = O.cnn_closed_form_params(seed=0)
    return CNN


def selector(L, P, cnn=True):
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_camera_params(P)
    if cnn:
        sel.set_cnn_state_dict(cnn_params())
    return sel


def dense_call(L, sel, labels, ids, depth, label_aware):
    """lg_select_grasp_labels with every plane and the validity plane taken back: (planes by name [B,H,W], validity, row bytes)"""
    from leafgrasp_amd import _lib

    lab = torch.from_numpy(np.ascontiguousarray(labels)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    B, H, W = lab.shape
    p = _lib.LgParams.from_buffer_copy(sel._sync_params(None))
    p.mask_is_bool = 1
    p.label_aware = 1 if label_aware else 0
    maps, ptrs = sel._alloc_maps(B, H, W)
    maps.fill_(float("nan"))
    valid = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    res = (_lib.LgGraspResult * B)()
    idv = (C.c_int32 * B)(*ids)
    rc = _lib.lib.lg_select_grasp_labels(sel._h, d.data_ptr(), lab.data_ptr(), idv, B, H, W, C.byref(p), C.byref(ptrs), valid.data_ptr(),
                                         res, sel._stream())
    _lib.check(sel._h, rc, "lg_select_grasp_labels")
    return {n: maps[i].cpu().numpy() for i, n in enumerate(_lib.MAP_NAMES)}, valid.cpu().numpy(), bytes(res), res


# (name, H, W, blobs (id, cx, cy, rx, ry), leaf id): the current leaf spans x 24..76 in the first three
CASES = [
    ("nearer than 15 px", 96, 128, [(1, 50, 48, 26, 24), (2, 88, 48, 6, 8)], 1),
    ("between 15 and 20 px: the wide term alone", 96, 128, [(1, 50, 48, 26, 24), (2, 99, 48, 6, 8)], 1),
    ("beyond 20 px, W % 16 != 0", 100, 150, [(1, 50, 50, 26, 24), (2, 120, 50, 8, 8), (3, 140, 90, 5, 5)], 1),
    ("every frame edge, the leaf on an edge", 160, 224,
     [(1, 10, 80, 40, 36), (2, 112, 2, 10, 6), (3, 221, 80, 6, 10), (4, 112, 158, 10, 5), (5, 2, 20, 5, 5)], 1),
    ("negative labels are background", 96, 128, [(1, 50, 48, 26, 24), (2, 88, 48, 6, 8), (-3, 30, 10, 12, 6), (-1, 110, 85, 9, 7)], 1),
    ("absent leaf id", 96, 128, [(1, 50, 48, 26, 24), (2, 88, 48, 6, 8)], 7),
]


@pytest.mark.parametrize("name,H,W,blobs,leaf", CASES, ids=[c[0] for c in CASES])
def test_transforms_and_plane(L, name, H, W, blobs, leaf):
    labels = R.blob_labels(H, W, blobs)
    if "negative" in name:
        assert (labels < 0).sum() > 50
    depth = depth_of(H, W)
    sel = selector(L, P_of(600.0, W / 2.0, H / 2.0))
    planes0, valid0, _, res0 = dense_call(L, sel, labels[None], [leaf], depth[None], False)
    planes1, valid1, _, res1 = dense_call(L, sel, labels[None], [leaf], depth[None], True)
    cur, oth, _ = R.split(labels, leaf)
    assert oth.any()
    got = sel.isolation_fields(0, H, W)
    assert got is not None
    _, (dcf, dwf) = R.transforms(oth)
    assert np.array_equal(got[0], dcf), ("dc", np.argwhere(got[0] != dcf)[:4])
    assert np.array_equal(got[1], dwf), ("dw", np.argwhere(got[1] != dwf)[:4])
    assert got[2] == (int(dcf.max()), int(dwf.max()))
    want = R.isolation_plane(labels, leaf)
    np.testing.assert_allclose(planes1["isolation_map"][0], want, rtol=1e-4, atol=1e-6)
    if cur.any():
        assert not np.array_equal(planes1["isolation_map"][0], planes0["isolation_map"][0]), "the plane must see the neighbour"
        if "wide term" in name:   # dc has a zero only inside the 30 ellipse: 17 px away the close term's transform is positive
            assert dcf[cur > 0].min() > 0 and dwf[cur > 0].min() == 0
    else:
        # no pixel carries the id: the current leaf is empty and every leaf is another leaf.  The C entry keeps what an empty
        # mask gives with the flag off (the reference's zero-score fall-through picks); the Python entry
        # reports found = 0 for a frame without a leaf id (None), in both modes
        assert (res1[0].found, res1[0].x, res1[0].y, res1[0].n_candidates) == (res0[0].found, res0[0].x, res0[0].y, res0[0].n_candidates)
        lab, d = torch.from_numpy(labels[None]).cuda(), torch.from_numpy(depth[None]).cuda()
        assert sel.select_grasp_points_for_leaves(lab, [None], d, label_aware=True) == [(None, None, None)]
        assert sel.last_results[0].found == 0
        t, c = sel.select_grasp_candidates_for_leaves(lab, [None], d, label_aware=True)
        assert t == [(None, None, None)] and (c["index"] == -1).all()
    for n in planes0:   # nothing else reads isolation
        if n != "isolation_map":
            assert planes1[n].tobytes() == planes0[n].tobytes(), n
    assert valid1.tobytes() == valid0.tobytes()


def test_others_cover_everything_but_the_leaf(L):
    H, W = 96, 128
    labels = np.full((H, W), 2, np.int16)
    labels[R.blob_labels(H, W, [(1, 60, 48, 8, 8)]) == 1] = 1
    sel = selector(L, P_of(600.0, 64.0, 48.0))
    planes, _, _, _ = dense_call(L, sel, labels[None], [1], depth_of(H, W)[None], True)
    dc, dw, mx = sel.isolation_fields(0, H, W)
    assert mx == (0, 0) and not dc.any() and not dw.any()
    assert not planes["isolation_map"].any()
    assert not R.isolation_plane(labels, 1).any()


def test_empty_others_is_the_default_call(L):
    H, W = 160, 224
    labels = R.blob_labels(H, W, [(1, 120, 64, 46, 40), (-2, 30, 30, 12, 12)])
    depth = depth_of(H, W)
    sel = selector(L, P_of(600.0, 112.0, 80.0))
    p0, v0, r0, _ = dense_call(L, sel, labels[None], [1], depth[None], False)
    p1, v1, r1, _ = dense_call(L, sel, labels[None], [1], depth[None], True)
    assert sel.isolation_fields(0, H, W) is None
    for n in p0:
        assert p0[n].tobytes() == p1[n].tobytes(), n
    assert v0.tobytes() == v1.tobytes() and r0 == r1
    lab, d = torch.from_numpy(labels[None]).cuda(), torch.from_numpy(depth[None]).cuda()
    t0, c0 = sel.select_grasp_candidates_for_leaves(lab, [1], d)
    t1, c1 = sel.select_grasp_candidates_for_leaves(lab, [1], d, label_aware=True)
    assert t0 == t1 and c0.tobytes() == c1.tobytes() and (c0["index"] >= 0).sum() > 1
    assert sel.select_grasp_points_for_leaves(lab, [1], d) == sel.select_grasp_points_for_leaves(lab, [1], d, label_aware=True)


# the leaf at x 116..204 of a 160 x 224 frame, the optical centre far to the left: the probes walk left from the grasp point
PRE = [
    ("neighbour under the default point: fall-back", [(1, 160, 60, 44, 40), (2, 78, 60, 14, 14), (3, 40, 130, 12, 10)]),
    ("large neighbour: fall-back lands on it", [(1, 160, 60, 44, 40), (2, 70, 60, 26, 20), (3, 40, 130, 12, 10)]),
    ("small neighbour: the next clear step", [(1, 160, 60, 44, 40), (2, 79, 63, 3, 3), (3, 40, 130, 12, 10)]),
]


@pytest.mark.parametrize("name,blobs", PRE, ids=[c[0] for c in PRE])
def test_pre_grasp_sees_the_neighbour(L, name, blobs):
    H, W = 160, 224
    labels, depth, P = R.blob_labels(H, W, blobs), depth_of(H, W), P_of(600.0, -400.0, 60.0)
    sel = selector(L, P, cnn=False)
    lab, d = torch.from_numpy(labels[None]).cuda(), torch.from_numpy(depth[None]).cuda()
    (xy0, g0, pre0), = sel.select_grasp_points_for_leaves(lab, [1], d)
    (xy1, g1, pre1), = sel.select_grasp_points_for_leaves(lab, [1], d, label_aware=True)
    ref = R.LabelAwareRef(labels, 1)
    ref.set_camera_params(P)
    exy, eg, epre = ref.select(depth)
    assert xy0 == xy1 == exy and g0 == g1
    np.testing.assert_allclose(g1, eg, rtol=1e-5)
    np.testing.assert_allclose(pre1, epre, rtol=1e-5)
    ref0 = O.RefGraspPointSelector()
    ref0.set_camera_params(P)
    np.testing.assert_allclose(pre0, ref0.calculate_pre_grasp_point(eg, ref.current), rtol=1e-5)
    u0, v0 = ref0._project_point_to_2d(pre0)
    clear = O.dilate(ref.all, O.ellipse_se(31))
    assert clear[v0, u0] != 0, "the default point lies within the clearance of a neighbour"
    if "small" not in name:
        assert labels[v0, u0] == 2, "the default point lies on the neighbour"
    assert not np.allclose(pre0, pre1), "this test fails without the feature"
    step = np.hypot(pre1[0] - g1[0], pre1[1] - g1[1]) / np.hypot(g1[0], g1[1]) * np.linalg.norm(g1)
    assert abs(step - (0.09 if "small" in name else 0.10)) < 1e-4, step
    # every ranked candidate follows the same rule
    _, c1 = sel.select_grasp_candidates_for_leaves(lab, [1], d, label_aware=True)
    _, c0 = sel.select_grasp_candidates_for_leaves(lab, [1], d)
    rows = [r for r in c1[0] if r["index"] >= 0]
    assert len(rows) > 3 and c0[0]["x"].tolist() == c1[0]["x"].tolist()
    changed = 0
    for r, r0 in zip(rows, c0[0]):
        g = ref.get_3d_grasp_point((int(r["x"]), int(r["y"])), depth)
        np.testing.assert_allclose([r["pX"], r["pY"], r["pZ"]], ref.calculate_pre_grasp_point(g, ref.current), rtol=1e-5)
        np.testing.assert_allclose([r0["pX"], r0["pY"], r0["pZ"]], ref0.calculate_pre_grasp_point(g, ref.current), rtol=1e-5)
        changed += (r["pX"], r["pY"]) != (r0["pX"], r0["pY"])
    assert changed > 0


def test_cnn_channel_sparse_and_dense(L):
    H, W = 160, 224
    labels = R.blob_labels(H, W, [(1, 120, 64, 46, 40), (2, 188, 64, 12, 16), (3, 40, 30, 14, 10), (4, 60, 140, 20, 12)])
    depth, P = depth_of(H, W), P_of(600.0, 112.0, 80.0)
    sel = selector(L, P)
    lab, d = torch.from_numpy(labels[None]).cuda(), torch.from_numpy(depth[None]).cuda()
    ref = R.LabelAwareRef(labels, 1, cnn=lambda x: O.cnn_forward(cnn_params(), x))
    ref.set_camera_params(P)
    scores = ref._calculate_all_scores(ref.current, depth)
    iso = scores["isolation_map"]
    assert len(np.unique(np.round(iso[ref.current > 0], 4))) > 10

    def check_slot(slot, x, y, logit):
        want = ref.patch_features(ref.current, depth, scores, (x, y))
        got = sel.patch(slot)
        np.testing.assert_allclose(got[5], want[5], rtol=1e-4, atol=1e-4, err_msg=f"channel 5 at ({x}, {y})")
        assert abs(float(logit) - float(O.cnn_forward(cnn_params(), want[None])[0])) <= 1e-4

    # sparse mode, deferred planes: the candidates entry scores every candidate in its own slot
    _, cands = sel.select_grasp_candidates_for_leaves(lab, [1], d, label_aware=True)
    torch.cuda.synchronize()
    s = sel.cnn_survivors()
    rows = [r for r in cands[0] if r["index"] >= 0]
    assert len(rows) > 5
    xy = {int(r["index"]): (int(r["x"]), int(r["y"])) for r in rows}
    for i, (x, y) in xy.items():
        check_slot(i, x, y, s["logits"][i])
    # the reference's own pick with its channel 5
    (got,) = sel.select_grasp_points_for_leaves(lab, [1], d, label_aware=True)
    exp = ref.select(depth)
    assert got[0] == exp[0]
    # dense call: the gather reads the stored plane; survivors of the pruned pass
    dense_call(L, sel, labels[None], [1], depth[None], True)
    s = sel.cnn_survivors()
    n = int(s["counts"][0])
    assert n > 0
    for j in range(n):
        i = int(s["list"][j]) % K
        check_slot(j, xy[i][0], xy[i][1], s["logits"][j])


def _frames():
    H, W = 160, 224
    shared = R.blob_labels(H, W, [(1, 150, 60, 44, 40), (2, 79, 63, 8, 8), (3, 50, 120, 30, 26)])
    alone = R.blob_labels(H, W, [(1, 110, 70, 46, 40)])
    other = R.blob_labels(H, W, [(1, 60, 60, 40, 38), (4, 130, 60, 10, 30), (5, 200, 140, 12, 12)])
    labels = [shared, alone, shared, other, alone]
    ids = [1, 1, 3, 1, 1]
    depth = [depth_of(H, W, 0.45 + 0.01 * i) for i in range(5)]
    return np.stack(labels), ids, np.stack(depth)


@pytest.mark.parametrize("B", [3, 5])
def test_mixed_batch_equals_single_frames(L, B):
    labels, ids, depth = _frames()
    labels, ids, depth = labels[:B], ids[:B], depth[:B]
    sel = selector(L, P_of(600.0, -200.0, 60.0))
    lab, d = torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda()
    sel.select_grasp_points_for_leaves(lab, ids, d, label_aware=True)
    rows = bytes(sel.last_results)
    fields = [sel.isolation_fields(b, 160, 224) for b in range(B)]
    assert [f is None for f in fields] == [i in (1, 4) for i in range(B)]
    _, cands = sel.select_grasp_candidates_for_leaves(lab, ids, d, label_aware=True)
    dense = dense_call(L, sel, labels, ids, depth, True)
    n = len(rows) // B
    one = selector(L, P_of(600.0, -200.0, 60.0))
    for b in range(B):
        one.select_grasp_points_for_leaves(lab[b:b + 1], ids[b:b + 1], d[b:b + 1], label_aware=True)
        assert bytes(one.last_results) == rows[b * n:(b + 1) * n], b
        f1 = one.isolation_fields(0, 160, 224)
        assert (f1 is None) == (fields[b] is None)
        if f1 is not None:
            assert np.array_equal(f1[0], fields[b][0]) and np.array_equal(f1[1], fields[b][1]) and f1[2] == fields[b][2]
        _, c1 = one.select_grasp_candidates_for_leaves(lab[b:b + 1], ids[b:b + 1], d[b:b + 1], label_aware=True)
        assert c1[0].tobytes() == cands[b].tobytes(), b
        d1 = dense_call(L, one, labels[b:b + 1], ids[b:b + 1], depth[b:b + 1], True)
        assert d1[0]["isolation_map"][0].tobytes() == dense[0]["isolation_map"][b].tobytes(), b
        assert d1[2] == dense[2][b * n:(b + 1) * n], b


def test_default_call_after_a_label_aware_call(L):
    labels, ids, depth = _frames()
    sel = selector(L, P_of(600.0, -200.0, 60.0))
    lab, d = torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda()
    t0, c0 = sel.select_grasp_candidates_for_leaves(lab, ids, d)
    sel.select_grasp_points_for_leaves(lab, ids, d)
    r0 = bytes(sel.last_results)
    p0 = dense_call(L, sel, labels, ids, depth, False)
    ta, ca = sel.select_grasp_candidates_for_leaves(lab, ids, d, label_aware=True)
    dense_call(L, sel, labels, ids, depth, True)
    assert ca.tobytes() != c0.tobytes()
    t1, c1 = sel.select_grasp_candidates_for_leaves(lab, ids, d)
    sel.select_grasp_points_for_leaves(lab, ids, d)
    p1 = dense_call(L, sel, labels, ids, depth, False)
    assert t0 == t1 and c0.tobytes() == c1.tobytes() and bytes(sel.last_results) == p1[2] == p0[2] == r0
    for n in p0[0]:
        assert p0[0][n].tobytes() == p1[0][n].tobytes(), n
    with pytest.raises(RuntimeError):
        sel.isolation_fields(0, 160, 224)   # the default call reused the scratch: no fields to read


def test_mask_entries_refuse_the_mode(L):
    from leafgrasp_amd import _lib

    H, W = 96, 128
    labels = R.blob_labels(H, W, [(1, 50, 48, 26, 24), (2, 88, 48, 6, 8)])
    sel = selector(L, P_of(600.0, 64.0, 48.0), cnn=False)
    m = torch.from_numpy((labels == 1).astype(np.uint8)[None]).cuda()
    d = torch.from_numpy(depth_of(H, W)[None]).cuda()
    p = _lib.LgParams.from_buffer_copy(sel._sync_params(None))
    res = (_lib.LgGraspResult * 1)()
    rows = (_lib.LgGraspCandidate * K)()
    for v in (1, 2):
        p.label_aware = v
        assert _lib.lib.lg_select_grasp(sel._h, d.data_ptr(), m.data_ptr(), 1, H, W, C.byref(p), None, None, res, sel._stream()) == _lib.LG_ERR_INVALID
        assert b"label_aware" in _lib.lib.lg_last_error(sel._h)
        assert _lib.lib.lg_select_grasp_candidates(sel._h, d.data_ptr(), m.data_ptr(), 1, H, W, C.byref(p), res, rows,
                                                   sel._stream()) == _lib.LG_ERR_INVALID
        maps, ptrs = sel._alloc_maps(1, H, W)
        assert _lib.lib.lg_score_maps(sel._h, d.data_ptr(), m.data_ptr(), 1, H, W, C.byref(p), C.byref(ptrs), None, None,
                                      sel._stream()) == _lib.LG_ERR_INVALID
    lab = torch.from_numpy(labels[None]).cuda()
    p.label_aware = 2
    ids = (C.c_int32 * 1)(1)
    assert _lib.lib.lg_select_grasp_labels(sel._h, d.data_ptr(), lab.data_ptr(), ids, 1, H, W, C.byref(p), None, None, res,
                                           sel._stream()) == _lib.LG_ERR_INVALID
