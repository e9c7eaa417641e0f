"""The collecting selector on the device (lg_select_grasp_collect and its stages; -m gpu), against tests/collect_ref.py:

  erosion     lg_erode_ellipse bit for bit against the erosion composed from the oracle's dilation: k in {3, 5, 15, 21, 63},
              one and two passes, 104 x 264 and 104 x 263, three frames per call (one empty), and 8 x 8 where everything erodes.
  tip         lg_tip_penalty as written at rtol 1e-4 / atol 1e-6 (the float planes' tolerance everywhere in this suite) on a leaf
              in the interior and one cut by the bottom-right corner, 120 x 168 and 121 x 167, both INIT_DIST0 values.
              tip_aware = 1 is not built: the entry refuses it (LG_ERR_UNSUPPORTED).
  arg-max     lg_argmax_first exactly np.argmax / np.max / (plane > 0).any() on handed planes.
  entry       three seeded 240 x 320 frames: safe, valid, distance_map and stem_penalty bit for bit, float planes at 1e-4 / 1e-6;
              the grasp pixel is the reference's wherever the reference's margin between its maximum and the next value is at
              least 4e-4 (four times the plane tolerance: two planes' worth of error on either side of a comparison, doubled),
              which the test computes and asserts for at least two seeds; for every seed the reference's score at the device's
              pixel is within 2e-4 relative of the reference's maximum.  3-D and pre-grasp points at 1e-5, the pre-grasp that of
              the ERODED mask.  A batch equals the single calls; a call that takes no output back gives the same rows.
  fallbacks   no valid pixel, and valid pixels that are all stem: the centroid of the ORIGINAL mask with n_candidates 0 (means
              clear of a knife edge, asserted); an empty mask: found 0 and the None triple.
  collector   CollectingGraspPointSelector.select_grasp_point with an EnhancedGraspDataCollector: the stored samples are the
              replay of collect_sample on the planes the entry returns, bit for bit (the tolerances of
              test_gpu_collect_sample.py), and equal the replay on the composed planes to the planes' own tolerances."""
import functools
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collect_ref as CR  # noqa: E402
import collector_cases as CC  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402

RTOL, ATOL = 1e-4, 1e-6
EXACT = ("distance_map", "stem_penalty")
MARGIN = 4e-4


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


@pytest.fixture(scope="module")
def sel(L):
    return L.CollectingGraspPointSelector(torch.device("cuda:0"))


def rows_of(s):
    """the last call's lg_grasp_result rows as bytes-comparable tuples"""
    return [tuple(getattr(r, n) for n, _ in r._fields_) for r in s.last_results]


# ------------------------------------------------------------------------------------------------ erosion
@functools.lru_cache(maxsize=None)
def _erosion_frames(W):
    m = CR.erosion_masks(104, W)
    return (np.stack([m["ellipse"], m["empty"], m["corner"]]), np.stack([m["hole"], m["full"], m["ellipse"]]))


@pytest.mark.parametrize("W", [264, 263])
@pytest.mark.parametrize("k,iterations", [(3, 1), (3, 2), (5, 2), (15, 1), (21, 1), (21, 2), (63, 1)])
def test_erode_ellipse(sel, W, k, iterations):
    for frames in _erosion_frames(W):
        got = sel.erode(torch.from_numpy(frames).cuda(), k, iterations).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(got[b], CR.erode(frames[b], k, iterations), err_msg=f"frame {b}")
        assert not got[1].any() or frames[1].all()   # the empty frame stays empty, the full one full


def test_erode_ellipse_at_the_smallest_frame(sel):
    m = np.ones((3, 8, 8), np.uint8)
    m[0, 3, 4] = 0        # one hole: the 21 ellipse reaches every pixel from it
    m[2] = 0
    got = sel.erode(torch.from_numpy(m).cuda(), 21, 2).cpu().numpy()
    for b in range(3):
        np.testing.assert_array_equal(got[b], CR.erode(m[b], 21, 2))
    assert not got[0].any() and got[1].all() and not got[2].any()


def test_erode_ellipse_refusals(L, sel):
    m = torch.zeros((1, 16, 16), dtype=torch.uint8, device="cuda:0")
    for k, it in ((20, 1), (65, 1), (0, 1), (21, 9), (21, -1)):
        with pytest.raises(L.LgError, match="status -5"):
            sel.erode(m, k, it)


# ------------------------------------------------------------------------------------------------ tip penalty
@pytest.mark.parametrize("shape", [(120, 168), (121, 167)])
@pytest.mark.parametrize("init0", [O.INIT_DIST0, 2 ** 31 - 1])
def test_tip_penalty_as_written(sel, shape, init0):
    H, W = shape
    safe = np.stack([CR.rotated_ellipse(H, W, W * 0.5, H * 0.45, W * 0.3, H * 0.3, 0.5),
                     CR.rotated_ellipse(H, W, W - 10, H - 8, W * 0.3, H * 0.35, -0.4)])
    assert safe[1, H - 1, W - 1] and not safe[0, 0, :].any()
    sel.params.chamfer_init_dist0 = init0
    try:
        got = sel.tip_penalty(torch.from_numpy(safe).cuda()).cpu().numpy()
    finally:
        sel.params.chamfer_init_dist0 = O.INIT_DIST0
    for b in range(2):
        exp = CR.tip_penalty_as_written(safe[b], init0)
        print(f"tip {shape} init0 {init0} frame {b}: max |diff| {np.max(np.abs(got[b] - exp)):.3e}, plane max {exp.max():.5f}")
        np.testing.assert_allclose(got[b], exp, rtol=RTOL, atol=ATOL)
        assert not got[b][safe[b] == 0].any()


def test_tip_aware_is_refused(L, sel):
    safe = torch.ones((1, 16, 16), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(L.LgError, match="status -5"):
        sel.tip_penalty(safe, tip_aware=True)
    mask, depth, P = CR.entry_scene(1)
    sel.set_camera_params(P)
    got = sel.select_grasp_point(torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(depth).cuda(), None, tip_aware=True)
    assert got == (None, None, None)


# ------------------------------------------------------------------------------------------------ arg-max
def _argmax_planes(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    base = rng.uniform(-1.0, 0.9, (H, W)).astype(np.float32)
    out = {}
    p = base.copy(); p[H - 1, W - 1] = 2.0
    out["unique maximum in the last pixel"] = p
    p = base.copy(); p[H // 2, W // 3] = 1.5; p[H // 2, W // 3 + 2] = 1.5; p[H - 1, 0] = 1.5
    out["equal maxima: the first wins"] = p
    out["all zero"] = np.zeros((H, W), np.float32)
    p = -np.abs(base) - 0.5; p[H // 3, W // 2] = -0.25
    out["all negative"] = p
    p = base.copy(); p[H // 2, W // 2] = 3.0; p[1, 2] = np.nan; p[H - 2, W - 3] = np.nan
    out["a NaN before and after the maximum"] = p
    p = np.zeros((H, W), np.float32); p[2, 1] = -0.0; p[H - 1, 3] = 0.0
    out["signed zeros"] = p
    p = base.copy(); p[3, 3] = np.inf; p[0, 0] = -np.inf
    out["infinities"] = p
    return out


@pytest.mark.parametrize("shape", [(8, 8), (104, 263)])
def test_argmax_first(sel, shape):
    H, W = shape
    planes = _argmax_planes(H, W)
    names = list(planes)
    for i in range(0, len(names), 3):     # B = 3 (the last call 1): differing frames in one call
        chunk = names[i:i + 3]
        stack = np.stack([planes[n] for n in chunk])
        xy, mx, anyp = sel.argmax_first(torch.from_numpy(stack).cuda())
        for b, n in enumerate(chunk):
            idx = int(np.argmax(stack[b]))
            assert xy[b] == (idx % W, idx // W), n
            assert anyp[b] == bool((stack[b] > 0).any()), n
            np.testing.assert_array_equal(np.float32(mx[b]), np.max(stack[b]), err_msg=n)   # (NaN equals NaN here)


# ------------------------------------------------------------------------------------------------ the whole entry
@functools.lru_cache(maxsize=None)
def _entry(seed):
    mask, depth, P = CR.entry_scene(seed)
    return mask, depth, P, CR.compose(mask, depth, P)


def _check_point(got, ref):
    np.testing.assert_allclose(got[1], ref["point_3d"], rtol=1e-5)
    np.testing.assert_allclose(got[2], ref["pre_grasp"], rtol=1e-5)


def test_whole_entry_against_the_composed_reference(sel):
    held = 0
    for seed in (1, 2, 3):
        mask, depth, P, ref = _entry(seed)
        sel.set_camera_params(P)
        out, planes, valid, safe = sel.select_grasp_points_batch(torch.from_numpy(mask[None]).cuda(), torch.from_numpy(depth[None]).cuda(),
                                                                 return_maps=True)
        row = sel.last_results[0]
        np.testing.assert_array_equal(safe[0].cpu().numpy(), ref["safe"])
        np.testing.assert_array_equal(valid[0].cpu().numpy().astype(bool), ref["valid"])
        for name, exp in ref["scores"].items():
            got = planes[name][0].cpu().numpy()
            if name in EXACT:
                np.testing.assert_array_equal(got, exp, err_msg=name)
            else:
                np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL, err_msg=f"{name} seed {seed}")
        trad = ref["scores"]["traditional_score"]
        m = CR.margin(trad)
        (x, y) = out[0][0]
        gap = (ref["best_score"] - float(trad[y, x])) / ref["best_score"]
        print(f"seed {seed}: reference margin {m:.3e}, device pixel {(x, y)} reference pixel {ref['point']}, score gap {gap:.3e}, "
              f"best {row.best_score:.6f} / {ref['best_score']:.6f}")
        assert ref["by_argmax"] and gap <= 2e-4
        if m >= MARGIN:
            held += 1
            assert (x, y) == ref["point"]
            _check_point(out[0], ref)
        assert (row.found, row.n_candidates, row.ml_used) == (1, 1, 0)
        np.testing.assert_allclose(row.best_score, ref["best_score"], rtol=RTOL)
        np.testing.assert_allclose(row.theta, ref["theta"], rtol=1e-4)
        assert float(planes["traditional_score"][0].max()) == row.best_score   # np.max of the plane the call returns
    assert held >= 2


def test_batch_equals_single_calls_and_outputs_do_not_change_the_rows(sel):
    frames = [_entry(seed) for seed in (1, 2, 3)]
    sel.set_camera_params(frames[0][2])
    single = []
    for mask, depth, _, _ in frames:
        sel.select_grasp_points_batch(torch.from_numpy(mask[None]).cuda(), torch.from_numpy(depth[None]).cuda())
        single += rows_of(sel)
    masks = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    depths = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    sel.select_grasp_points_batch(masks, depths)
    assert rows_of(sel) == single
    sel.select_grasp_points_batch(masks, depths, return_maps=True)
    assert rows_of(sel) == single


def test_python_triple_of_one_frame(sel):
    mask, depth, P, ref = _entry(2)
    sel.set_camera_params(P)
    got = sel.select_grasp_point(torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(depth).cuda(), None)
    assert got[0] == ref["point"]
    _check_point(got, ref)
    assert sel.select_grasp_point(torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(depth).cuda(), None,
                                  pcl_data=[(0.0, 0.0, 0.0)]) == (None, None, None)   # quirk 10


# ------------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("scene,valid_px", [((240, 320, 3), 0), ((720, 960, 11), 2861)])
def test_centroid_fallback(sel, scene, valid_px):
    mask, depth, P = CR.largest_leaf(*scene)
    ref = CR.compose(mask, depth, P)
    pt, frac = CR.centroid(mask)
    assert int(ref["valid"].sum()) == valid_px and not ref["by_argmax"] and ref["point"] == pt
    assert all(0.05 <= f <= 0.95 for f in frac), frac     # clear of a knife edge: every rounding of the mean truncates alike
    if valid_px:
        assert (ref["scores"]["stem_penalty"][ref["valid"]] == 1).all()   # valid pixels, all under the stem penalty
    sel.set_camera_params(P)
    out = sel.select_grasp_points_batch(torch.from_numpy(mask[None]).cuda(), torch.from_numpy(depth[None]).cuda())
    row = sel.last_results[0]
    assert out[0][0] == pt and (row.found, row.n_candidates, row.ml_used) == (1, 0, 0) and row.best_score == 0.0
    _check_point(out[0], ref)


def test_empty_mask(sel):
    mask, depth, P, _ = _entry(1)
    sel.set_camera_params(P)
    masks = np.stack([np.zeros_like(mask), mask])
    out = sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), torch.from_numpy(np.stack([depth, depth])).cuda())
    assert out[0] == (None, None, None) and sel.last_results[0].found == 0
    assert out[1][0] == _entry(1)[3]["point"]
    assert sel.select_grasp_point(torch.zeros(mask.shape, dtype=torch.bool).cuda(), torch.from_numpy(depth).cuda(), None) == (None,) * 3


# ------------------------------------------------------------------------------------------------ collector link
def test_collector_receives_the_variants_planes(L, tmp_path):
    mask, depth, P, ref = _entry(1)
    col = L.EnhancedGraspDataCollector(patch_size=32, resume=False, data_dir=str(tmp_path), device="cuda:0")
    s = L.CollectingGraspPointSelector(torch.device("cuda:0"), data_collector=col)
    s.set_camera_params(P)
    mt, dt = torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(depth).cuda()
    _, planes, _, _ = s.select_grasp_points_batch(mt, dt, return_maps=True)
    handed = {k: planes[k][0].cpu().numpy() for k in O.SCORE_KEYS}
    total = float(s.last_results[0].best_score)
    random.seed(7)
    got = s.select_grasp_point(mt, dt, None)
    assert got[0] == ref["point"]
    samples = col.samples
    # bit for bit: the replay of collect_sample on the planes the entry hands over
    exp = CC.replay_collect_sample(mask, depth, handed, got[0], total, 7)
    assert exp is not None and [smp["grasp_point"] for smp in samples] == [tuple(e[1]) for e in exp]
    for smp, (p, _, tot, lab, _) in zip(samples, exp):
        assert smp["label"] == lab and abs(smp["total_score"] - tot) < 1e-12
        np.testing.assert_array_equal(smp["mask_patch"].numpy(), p[1])
        np.testing.assert_array_equal(smp["score_patches"].numpy(), p[2])
        if not smp["is_augmented"]:
            np.testing.assert_array_equal(smp["depth_patch"].numpy(), p[0])
    # and the composed planes, to the planes' tolerances
    composed = {k: np.asarray(ref["scores"][k], np.float32) for k in O.SCORE_KEYS}
    expc = CC.replay_collect_sample(mask, depth, composed, ref["point"], ref["best_score"], 7)
    assert [smp["grasp_point"] for smp in samples] == [tuple(e[1]) for e in expc]
    for smp, (p, _, tot, lab, _) in zip(samples, expc):
        assert smp["label"] == lab
        np.testing.assert_allclose(smp["total_score"], tot, rtol=RTOL)
        np.testing.assert_array_equal(smp["mask_patch"].numpy(), p[1])
        sp = smp["score_patches"].numpy()
        np.testing.assert_allclose(sp, p[2], rtol=RTOL, atol=ATOL)
        for name in EXACT:
            ch = O.SCORE_KEYS.index(name)
            np.testing.assert_array_equal(sp[ch], p[2][ch])
    assert col.stats["positive_samples"] == 1 and col.stats["negative_samples"] == sum(1 for e in exp if e[3] == 0) > 0
