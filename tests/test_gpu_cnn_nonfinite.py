"""Non-finite values through the CNN kernels and the patch gather, against the oracle.

torch's relu and max_pool2d propagate NaN, so one NaN or infinity anywhere in a patch makes the reference's logit of that
patch NaN and leaves every other patch of the batch as it was.  The device must do the same: `np.isnan(logit)` exactly at the
poisoned positions, and every clean position equal, bit for bit, to the same call at the same N (the same plan, the same
summation order) with the poisoned patches replaced by their clean originals -- a NaN must not cross into another patch through
a shared work item, a split item's partial sums, the zero planes 9-11, a halo or the head.

Batch position i holds patch i % M of a prime pool; patch p of the pool has ONE poisoned version: value VALUES[p % 4] in
channel p % 9 at pixel PIXELS[p % 13] (9, 13 and 4 are pairwise coprime: every pair of them occurs within the pool).  A
pattern says which positions of a batch take the poisoned version.

The gather (lg_gather_kernel): a channel that holds a NaN comes out raw as the reference's `if p.max() > p.min()` leaves it, a
channel with an infinity as NumPy's arithmetic gives it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import cnn_plan as C  # noqa: E402
from tests.test_gpu_cnn_regimes import ATOL, FORMS, RTOL, STANDARD, VARIANTS, _load_with_env, _params, _pool  # noqa: E402

M = 211            # a prime: the pool of distinct patches
SEED = 41
NEG_NAN = np.frombuffer(np.uint32(0xFFC00000).tobytes(), np.float32)[0]    # NaN with the sign bit set
VALUES = (np.float32(np.nan), NEG_NAN, np.float32(np.inf), np.float32(-np.inf))
# the corners, one interior pixel, and both sides of the F(4x4) tile / 2x2 pool boundaries at rows and columns 3|4 and 15|16
PIXELS = ((0, 0), (31, 31), (0, 31), (31, 0), (13, 18), (3, 3), (3, 4), (4, 3), (4, 4), (15, 15), (15, 16), (16, 15), (16, 16))


def _spec(p):
    """(channel, row, column, value) of pool patch p's poisoned version."""
    return (p % 9,) + PIXELS[p % 13] + (VALUES[p % 4],)


@functools.lru_cache(maxsize=None)
def _poisoned_pool():
    x = _pool(M, SEED).copy()
    for p in range(M):
        c, y, xx, v = _spec(p)
        x[p, c, y, xx] = v
    return x


@functools.lru_cache(maxsize=None)
def _pools_dev():
    return torch.from_numpy(_pool(M, SEED)).cuda(), torch.from_numpy(_poisoned_pool()).cuda()


@functools.lru_cache(maxsize=None)
def _oracle_logits(name):
    """float64 logits of the clean pool, after the oracle-only precondition: NaN for every poisoned patch, finite for every
    clean one.  Before any device call of the model."""
    clean = O.cnn_forward(_params(name), _pool(M, SEED), dtype=torch.float64)
    bad = O.cnn_forward(_params(name), _poisoned_pool(), dtype=torch.float64)
    assert np.isfinite(clean).all(), name
    assert np.isnan(bad).all(), (name, [_spec(p) for p in np.nonzero(~np.isnan(bad))[0]])
    return clean


def _patterns(n):
    """name -> bool [n], the poisoned positions: every 7th (poisoned and clean patches inside every work item), the same with
    the batch's highest index (left-over items compute the highest indices), and a run of consecutive patches (70 of them from
    N = 140 on: longer than one item, which holds at most 32 patches -- 32 tiles of the deep encoder's 4 x 4 layers)."""
    i = np.arange(n)
    every7 = i % 7 == 3
    last = every7 | (i == n - 1)
    run = (i >= n // 4) & (i < n // 4 + min(max(n // 2, 1), 70))
    out = {"every 7th": every7, "every 7th and the last": last, "run": run}
    return {k: v for k, v in out.items() if v.any()}


def _covered(n):
    specs = [_spec(int(i) % M) for i in np.nonzero(_patterns(n)["every 7th"])[0]]
    return ({s[0] for s in specs}, {s[1:3] for s in specs}, {np.float32(s[3]).view(np.uint32).item() for s in specs})


def _counts(filters, num_cu):
    """1, 20, 640 and the smallest count whose plan splits a left-over item over P = 2, 4 and 8 workgroups, as far as this
    device's plans reach them."""
    _, first = C.pick_counts(C.model_layers(filters), num_cu)
    split = {}
    for (_, c), n in first.items():
        if c[2] > 1:
            split[c[2]] = min(n, split.get(c[2], n))
    assert all(n <= 640 for n in split.values()), split
    return sorted({1, 20, 640} | set(split.values())), split


def _check(sel, name, counts, what):
    ref = _oracle_logits(name)            # (cached: computed before the first device call of this model)
    clean_pool, bad_pool = _pools_dev()
    for n in counts:
        idx = torch.arange(n, device="cuda") % M
        x_clean = clean_pool[idx]
        base = sel.cnn_forward(x_clean).cpu().numpy()
        np.testing.assert_allclose(base, ref[np.arange(n) % M], rtol=RTOL, atol=ATOL, err_msg=f"{what}: N {n}, clean batch")
        for pname, bad in _patterns(n).items():
            x = x_clean.clone()
            sel_bad = torch.from_numpy(bad).cuda()
            x[sel_bad] = bad_pool[idx[sel_bad]]
            got = sel.cnn_forward(x).cpu().numpy()
            msg = f"{what}: N {n}, {pname} ({int(bad.sum())} poisoned)"
            wrong = np.nonzero(np.isnan(got) != bad)[0]
            assert wrong.size == 0, (msg, "NaN logits differ from the poisoned positions at", wrong[:10].tolist(),
                                     [_spec(int(i) % M) for i in wrong[:10]], got[wrong[:10]].tolist())
            np.testing.assert_array_equal(got[~bad].view(np.uint32), base[~bad].view(np.uint32),
                                          err_msg=msg + ": clean positions against the all-clean call")
            np.testing.assert_allclose(got[~bad], ref[np.arange(n) % M][~bad], rtol=RTOL, atol=ATOL, err_msg=msg)


@pytest.fixture(scope="module")
def sel():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    yield s
    s.clear_cnn()


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


def test_the_poisoned_patches_cover_the_placements():
    """Between them the poisoned patches of the 640-patch batch cover every channel, every pixel of PIXELS and the four values;
    the pool itself holds every (channel, pixel), (pixel, value) and (channel, value) pair."""
    chans, pixels, values = _covered(640)
    assert chans == set(range(9)) and pixels == set(PIXELS) and len(values) == 4
    specs = [_spec(p) for p in range(M)]
    assert len({(s[0], s[1:3]) for s in specs}) == 9 * 13 and len({(s[0], p % 4) for p, s in enumerate(specs)}) == 36
    assert len({(s[1:3], p % 4) for p, s in enumerate(specs)}) == 52
    assert np.isnan(NEG_NAN) and np.signbit(NEG_NAN) and not np.signbit(VALUES[0])
    pats = _patterns(640)
    assert pats["every 7th and the last"][639] and not pats["every 7th"][639] and pats["run"].sum() == 70
    assert all(p.mean() < 0.2 for p in pats.values())      # most patches stay clean


def test_standard_model_default_path(sel, num_cu):
    _oracle_logits("standard")
    counts, split = _counts(STANDARD, num_cu)
    if num_cu == 256:
        assert set(split) == {2, 4, 8}, split
    sel.set_cnn_state_dict(_params("standard"))
    _check(sel, "standard", counts, "standard")
    sel.clear_cnn()


@pytest.mark.parametrize("form,env", FORMS, ids=[f for f, _ in FORMS])
def test_conv_forms(sel, monkeypatch, num_cu, form, env):
    _oracle_logits("standard")
    counts, _ = _counts(STANDARD, num_cu)
    _load_with_env(sel, monkeypatch, _params("standard"), env)
    _check(sel, "standard", counts, form)
    sel.clear_cnn()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants(sel, num_cu, name):
    _oracle_logits(name)
    counts, _ = _counts(VARIANTS[name][2], num_cu)
    sel.set_cnn_state_dict(_params(name))
    _check(sel, name, counts, name)
    sel.clear_cnn()


# ----------------------------------------------------------------------------------------------------------- the gather
GH, GW = 96, 128
INTERIOR, CORNER0, CORNER1 = (64, 48), (3, 2), (GW - 2, GH - 3)      # (x, y): the two corner windows are replicate-padded
CHANNELS = ("depth", "mask") + tuple(n for n in ("sdf_score", "approach_score", "flatness_map", "isolation_map", "distance_map",
                                                 "accessibility_map", "stem_penalty"))


@functools.lru_cache(maxsize=None)
def _gather_scene():
    _, depth, P = O.synthetic_scene(GH, GW, 5)
    yy, xx = np.mgrid[:GH, :GW]
    mask = (((xx - 60) / 50.0) ** 2 + ((yy - 46) / 34.0) ** 2 <= 1.0).astype(np.uint8)
    mask[:6, :8] = 1                      # leaf pixels under both corner windows
    mask[GH - 7:, GW - 9:] = 1
    return mask, depth.astype(np.float32), P


# name -> [(row, column, value)]: holes on the leaf inside the interior window (rows 32..63, columns 48..79) and at the two
# frame corners (pixel (0, 0) is replicated over the whole padding of its window)
GATHER_CASES = {
    "none": [],
    "nan": [(40, 60, np.nan), (0, 0, np.nan), (GH - 1, GW - 1, np.nan)],
    "inf": [(40, 60, np.inf), (0, 0, np.inf), (GH - 1, GW - 1, np.inf)],
    "both": [(40, 60, np.nan), (55, 70, np.inf), (0, 0, np.nan), (2, 3, np.inf), (GH - 1, GW - 1, np.inf), (GH - 4, GW - 3, np.nan)],
}


def _assert_patch(got, exp, what):
    for c, name in enumerate(CHANNELS):
        np.testing.assert_allclose(got[c], exp[c], rtol=1e-4, atol=1e-6, equal_nan=True, err_msg=f"{what}: channel {c} ({name})")


@pytest.mark.parametrize("case", list(GATHER_CASES))
def test_gather_against_patch_features(sel, case):
    """lg_gather_patches over the ORACLE's planes against RefGraspPointSelector.patch_features, channel by channel."""
    mask, depth, P = _gather_scene()
    d = depth.copy()
    for y, x, v in GATHER_CASES[case]:
        assert mask[y, x]
        d[y, x] = v
    ref = O.RefGraspPointSelector()
    ref.set_camera_params(P)
    with np.errstate(all="ignore"):
        sc = ref._calculate_all_scores(mask, d)
        pts = [INTERIOR, CORNER0, CORNER1]
        exp = [ref.patch_features(mask, d, sc, p) for p in pts]
    # what the expectation itself holds (oracle only): a window with a NaN keeps its depth channel raw, one with an infinity
    # alone is normalised by NumPy's arithmetic (0 at the finite pixels, NaN at the infinite one), a clean one lies in [0, 1]
    for e, p in zip(exp, pts):
        x, y = p
        win = ref._extract_local_patch(d, x, y)
        if np.isnan(win).any():
            assert np.array_equal(e[0], win, equal_nan=True), (case, p)
        elif np.isinf(win).any():
            assert np.isnan(e[0]).sum() == np.isinf(win).sum() and (e[0][~np.isnan(e[0])] == 0).all(), (case, p)
        else:
            assert e[0].min() == 0.0 and e[0].max() == 1.0, (case, p)
    maps = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for k, v in sc.items()}
    got = sel.gather_patches(torch.from_numpy(mask).cuda(), torch.from_numpy(d).cuda(), maps, pts).cpu().numpy()
    for i, p in enumerate(pts):
        _assert_patch(got[i], exp[i], f"{case} {p}")


@pytest.mark.parametrize("env", [{}, {"LG_DEFER_PLANES": "0"}], ids=["default", "LG_DEFER_PLANES=0"])
def test_staged_patches_against_patch_features(monkeypatch, env):
    """The patches the CNN read inside a select call with a model loaded (lg_debug_patch) against patch_features over the
    planes lg_score_maps gives for the same frame, for every candidate -- those whose window holds a hole among them."""
    import leafgrasp_amd

    from tests.test_gpu_nonfinite_select import frame_b

    mask, depth, holed, P, _ = frame_b()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    for k in env:
        monkeypatch.delenv(k)
    s.set_camera_params(P)
    s.set_cnn_state_dict(_params("standard"))
    m8, dd = torch.from_numpy(mask.astype(np.uint8)).cuda(), torch.from_numpy(holed).cuda()
    _, cands = s.select_grasp_candidates_batch(m8, dd)      # a uint8 mask: every candidate is scored, in its own slot
    rows = cands[0][cands[0]["index"] >= 0]
    maps, _, _ = s.score_maps(m8, dd)
    maps_np = {k: v.cpu().numpy() for k, v in maps.items()}
    ref = O.RefGraspPointSelector()
    n_holed = 0
    for r in rows:
        x, y = int(r["x"]), int(r["y"])
        with np.errstate(all="ignore"):
            exp = ref.patch_features(mask.astype(np.uint8), holed, maps_np, (x, y))
        n_holed += bool(np.isnan(exp[0]).any())
        _assert_patch(s.patch(int(r["index"])), exp, f"candidate {int(r['index'])} at {(x, y)}")
    assert 2 <= n_holed < len(rows), n_holed
    s.clear_cnn()
