"""The pruned CNN pass of lg_select_grasp, survivor by survivor, at every plan its device-side patch count can give.

The pruned pass launches every CNN layer on a grid sized for the host's bound B * top_k and lets the kernels recompute their
item plan from the survivor count the device wrote in front of them; tests/cnn_plan.py restates that plan (device_plan) and
composes batches whose (bound, count) pairs reach every class of every layer, the slice boundary at 8192 and counts that
fill no tile block.  lg_debug_cnn_survivors (GraspPointSelector.cnn_survivors) exports the pass: per call the survivor list,
the slot map, the count and the logits are held to

  * the candidates the exported predicate (lg_cnn_candidate_cannot_win) and the border rule keep, computed on the host from the
    rows of select_grasp_candidates_batch, frame-major in candidate order; the slot map inverts the list;
  * the logits of a handle created with LG_CNN_PRUNE=0, bit for bit (a logit does not depend on what runs beside it);
  * the float64 network (oracle.cnn_forward) on the candidate's dense patch from gather_patches, at the tolerance of
    tests/test_gpu_cnn_regimes.py;

and the result rows to the unpruned handle's and to a repeated call's, byte for byte.

Steering the count: masks are uint8 (every candidate is eligible).  An empty mask gives top_k survivors (all candidates tie at
the constant tile's score); a leaf frame gives one (candidate 0; the runner-up's best possible combined score stays 0.03 or
more below it, see _pool); a call with top_k = 1 gives none.  The leaf frames are windows of 384 x 512 scenes around their
largest leaf -- at 192 x 256 the scenes' own leaves are too narrow for a valid region.  Empty frames differ in their depth
(seven variants) and leaf frames in their scene (three), so a patch or logit taken from a neighbouring frame shows."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import cnn_plan as C  # noqa: E402
from tests.test_gpu_cnn_regimes import ATOL, RTOL  # noqa: E402

WEIGHTS = ("w_approach", "w_sdf", "w_flat", "w_access")
STANDARD = (64, 128, 256)
BIG, SMALL = (192, 256), (96, 128)
LEAF_SEEDS = (3, 4, 12)                    # scenes whose window holds exactly one survivor
EMPTY_SEEDS = (3, 4, 12, 6, 9, 11, 5)      # depth windows under the empty masks
worst = {"err": 0.0}                       # largest |logit - float64| / (ATOL + RTOL |float64|) seen by this module


# ------------------------------------------------------------------------------------------------------------- handles
def _selector(params):
    import leafgrasp_amd

    s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    s.set_cnn_state_dict(params)
    return s


def _handles(env):
    """One selector per entry of env (a dict of environment settings read at lg_create)."""
    mp = pytest.MonkeyPatch()
    out = []
    for e in env:
        for k in ("LG_CNN_PRUNE", "LG_SUBBATCH"):
            mp.delenv(k, raising=False)
        for k, v in e.items():
            mp.setenv(k, v)
        out.append(_selector(O.cnn_closed_form_params(seed=0)))
    mp.undo()
    return out


@pytest.fixture(scope="module")
def pair():
    """(default handle, handle created with LG_CNN_PRUNE=0)"""
    assert torch.cuda.is_available()
    on, off = _handles([{}, {"LG_CNN_PRUNE": "0"}])
    yield on, off
    print(f"\nworst logit error of the module, in units of the tolerance (atol {ATOL} + rtol {RTOL}): {worst['err']:.3f}")
    on.clear_cnn()
    off.clear_cnn()


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


# ---------------------------------------------------------------------------------------------------------------- pool
def _largest_leaf(labels):
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    return labels == ids[np.argmax(counts)]


@functools.lru_cache(maxsize=None)
def _window(seed, size):
    """(mask uint8, depth) of the size[0] x size[1] window around the largest leaf of the 384 x 512 scene `seed`."""
    labels, depth, _ = O.synthetic_scene(384, 512, seed)
    m = _largest_leaf(labels)
    ys, xs = np.nonzero(m)
    h, w = size
    y0 = min(max((int(ys.min()) + int(ys.max())) // 2 - h // 2, 0), 384 - h)
    x0 = min(max((int(xs.min()) + int(xs.max())) // 2 - w // 2, 0), 512 - w)
    return np.ascontiguousarray(m[y0:y0 + h, x0:x0 + w]).astype(np.uint8), np.ascontiguousarray(depth[y0:y0 + h, x0:x0 + w])


class Pool:
    """The distinct scenes of one frame size on the device -- leaf scenes first, then the empty ones -- and what the tests
    need of each, computed once: the candidates per top_k (from the candidates entry) and the float64 logit per candidate."""

    def __init__(self, size):
        self.size = size
        leaf = [_window(s, size) for s in LEAF_SEEDS]
        empty = [(np.zeros(size, np.uint8), _window(s, size)[1]) for s in EMPTY_SEEDS]
        self.n_leaf, self.n_empty = len(leaf), len(empty)
        self.masks = torch.from_numpy(np.stack([m for m, _ in leaf + empty])).cuda()
        self.depths = torch.from_numpy(np.stack([d for _, d in leaf + empty])).cuda()
        # the camera of a frame of this size (principal point inside the window: the approach and accessibility scores then
        # fall off around the leaf as they do in a whole frame, and the runner-up stays well below candidate 0)
        self.P = O.synthetic_scene(size[0], size[1], 0)[2]
        self._cands, self._ref, self._maps = {}, {}, {}

    def scene_ids(self, is_empty):
        """Frame -> scene: the leaf frames cycle through the leaf scenes, the empty ones through the depth variants."""
        is_empty = np.asarray(is_empty, bool)
        ids = np.empty(is_empty.size, np.int64)
        ids[~is_empty] = np.arange(int((~is_empty).sum())) % self.n_leaf
        ids[is_empty] = self.n_leaf + np.arange(int(is_empty.sum())) % self.n_empty
        return ids

    def frames(self, ids):
        """(masks, depths) of the frames whose scenes are ids, on the device."""
        i = torch.from_numpy(np.asarray(ids, np.int64)).cuda()
        return self.masks[i].contiguous(), self.depths[i].contiguous()

    def candidates(self, sel, k):
        """Per scene (x, y, traditional) arrays of its candidates at top_k = k in candidate order, from the candidates entry."""
        if k not in self._cands:
            _, cands = sel.select_grasp_candidates_batch(self.masks, self.depths, top_k=k)
            per = []
            for rows in cands:
                rows = rows[rows["index"] >= 0]
                rows = rows[np.argsort(rows["index"], kind="stable")]
                assert rows["index"].tolist() == list(range(len(rows)))
                per.append((rows["x"].astype(np.int64), rows["y"].astype(np.int64), rows["traditional"].astype(np.float64)))
            self._cands[k] = per
        return self._cands[k]

    def ref_logits(self, sel, scene, xs, ys, params):
        """float64 logits of the candidates (xs, ys) of a scene: the dense patches of gather_patches through the float64 network."""
        have = self._ref.setdefault(scene, {})
        need = [(int(x), int(y)) for x, y in zip(xs, ys) if (int(x), int(y)) not in have]
        if need:
            if scene not in self._maps:
                self._maps[scene] = sel.score_maps(self.masks[scene], self.depths[scene])[0]
            patches = sel.gather_patches(self.masks[scene], self.depths[scene], self._maps[scene], need)
            for p, v in zip(need, O.cnn_forward(params, patches.cpu().numpy(), dtype=torch.float64)):
                have[p] = float(v)
        return np.array([have[(int(x), int(y))] for x, y in zip(xs, ys)], np.float64)


@functools.lru_cache(maxsize=None)
def _other_params():
    return O.cnn_closed_form_params(seed=1)


@functools.lru_cache(maxsize=None)
def _pool(size):
    return Pool(size)


def _survivors(xs, ys, trad, H, W, is_bool=False):
    """Candidates of a frame that go through the CNN: none in a frame with one candidate; else those the rescoring scores
    (border rule of a torch.bool mask) and that the exported predicate does not rule out against candidate 0."""
    import leafgrasp_amd as L

    if len(xs) <= 1:
        return []
    keep = []
    for i, (x, y, t) in enumerate(zip(xs, ys, trad)):
        if is_bool and (x < 16 or y < 16 or x + 16 > W or y + 16 > H):
            continue
        if not L._lib.lib.lg_cnn_candidate_cannot_win(float(t), float(trad[0])):
            keep.append(i)
    return keep


def _spread(B, e):
    """B frames of which e are empty, the others spread evenly among them (first and last frame included where they fit)."""
    is_empty = np.ones(B, bool)
    n = B - e
    if n:
        is_empty[np.floor(np.linspace(0, B - 1, n) + 0.5).astype(int)] = False
        assert int((~is_empty).sum()) == n
    return is_empty


# ------------------------------------------------------------------------------------------------------------ the check
def _call(sel, pool, ids, k, repeat=True):
    """-> (result rows as bytes, export, lg_debug_cnn_scored) of select_grasp_points_batch at top_k = k; a repeated call gives
    the same."""
    m, d = pool.frames(ids)
    sel.set_camera_params(pool.P)
    sel.params.top_k = k
    try:
        sel.select_grasp_points_batch(m, d)
        rows, ex, scored = bytes(sel.last_results), sel.cnn_survivors(), sel.cnn_scored()
        if repeat:
            sel.select_grasp_points_batch(m, d)
            ex2 = sel.cnn_survivors()
            assert bytes(sel.last_results) == rows and sel.cnn_scored() == scored, "repeated call: rows"
            for f in ("counts", "list", "slot"):
                np.testing.assert_array_equal(ex2[f], ex[f], err_msg=f"repeated call: {f}")
    finally:
        sel.params.top_k = 20
    return rows, ex, scored


def _expected(pool, sel_for_cands, ids, k, sub_frames):
    """What the export of a pruned call must hold: (counts per sub-batch, list, slot, (frame, candidate) of every survivor in
    order, candidate count per frame)."""
    H, W = pool.size
    cands = pool.candidates(sel_for_cands, k)
    surv = {s: _survivors(*cands[s], H, W) for s in set(ids.tolist())}
    B = len(ids)
    lst, slot = np.full(B * k, -1, np.int32), np.full(B * k, -1, np.int32)
    counts, pairs = [], []
    for off in range(0, B, sub_frames):
        j = 0
        for b in range(off, min(off + sub_frames, B)):
            for i in surv[int(ids[b])]:
                lst[off * k + j] = (b - off) * k + i
                slot[b * k + i] = j
                pairs.append((b, i))
                j += 1
        counts.append(j)
    return np.array(counts, np.int32), lst, slot, pairs, np.array([len(cands[int(s)][0]) for s in ids])


def _check(pair, pool, is_empty, k, what, target=None, on=None, params=None, fill=True):
    """One batch through the pruned handle (`on`, default pair[0]) and the unpruned one: everything the module docstring lists.
    fill=False leaves out the fill of the logits buffer in front of the pruned call and with it the past-the-count check
    (test_small_call_after_a_large_one, which needs its calls back to back, makes that check itself).
    -> (rows, export of the pruned handle)."""
    off = pair[1]
    on = on or pair[0]
    params = params or O.cnn_closed_form_params(seed=0)
    ids = pool.scene_ids(is_empty)
    B = len(ids)
    rows_off, ex_off, scored_off = _call(off, pool, ids, k)
    # Before the pruned call the candidates entry (every candidate scored) fills all B * k logits of the pruned handle's buffer
    # under OTHER weights: the pruned pass then must leave the slots past its count as they are -- a pass that ran on more
    # patches than survived would put the standard weights' logits there.
    # (fill=False: the call follows the handle's previous one directly)
    before = None
    if fill:
        on.set_cnn_state_dict(_other_params())
        on.set_camera_params(pool.P)
        on.select_grasp_candidates_batch(*pool.frames(ids), top_k=k)
        before = on.cnn_survivors()
        assert int(before["counts"].sum()) == B * k
        on.set_cnn_state_dict(params)
    rows_on, ex_on, scored_on = _call(on, pool, ids, k)
    SB = ex_on["sub_frames"]
    counts, lst, slot, pairs, ncand = _expected(pool, off, ids, k, SB)
    print(f"{what}: B {B} top_k {k}: {int(counts.sum())} of {B * k} patches through the CNN, sub-batches {counts.tolist()}")
    if target is not None:
        assert int(counts.sum()) == target, (what, "the pool gives", int(counts.sum()), "survivors, not the target", target)
    # the unpruned handle: one sub-batch, the identity
    assert (ex_off["sub_frames"], ex_off["n_sub"], ex_off["counts"].tolist()) == (B, 1, [B * k]), what
    np.testing.assert_array_equal(ex_off["list"], np.arange(B * k), err_msg=what)
    np.testing.assert_array_equal(ex_off["slot"], np.arange(B * k), err_msg=what)
    assert scored_off == B * k
    # the pruned handle: count, list, slot map
    assert ex_on["n_sub"] == len(counts) and ex_on["counts"].tolist() == counts.tolist(), (what, ex_on["counts"], counts)
    np.testing.assert_array_equal(ex_on["list"], lst, err_msg=f"{what}: survivor list")
    np.testing.assert_array_equal(ex_on["slot"], slot, err_msg=f"{what}: slot map")
    assert scored_on == int(counts.sum())
    # every survivor's logit: the unpruned handle's for that candidate, bit for bit, and the float64 network's
    pb = np.array([b for b, _ in pairs], np.int64)
    pi = np.array([i for _, i in pairs], np.int64)
    if len(pairs):
        pos = (pb // SB) * SB * k + slot[pb * k + pi]
        got = ex_on["logits"][pos]
        np.testing.assert_array_equal(got.view(np.uint32), ex_off["logits"][pb * k + pi].view(np.uint32),
                                      err_msg=f"{what}: pruned against unpruned logits")
    # ... float64: of every candidate slot the unpruned pass filled (the survivors are among them, bit-equal)
    ref = np.full(B * k, np.nan)
    for s in set(ids.tolist()):
        xs, ys, _ = pool.candidates(off, k)[s]
        r = pool.ref_logits(off, s, xs, ys, params)
        for b in np.nonzero(ids == s)[0]:
            ref[b * k:b * k + len(r)] = r
    have = ~np.isnan(ref)
    assert have.sum() == ncand.sum()
    err = np.abs(ex_off["logits"][have] - ref[have]) / (ATOL + RTOL * np.abs(ref[have]))
    worst["err"] = max(worst["err"], float(err.max()))
    print(f"{what}: largest logit error {float(err.max()):.3f} of the tolerance over {int(have.sum())} candidates")
    np.testing.assert_allclose(ex_off["logits"][have], ref[have], rtol=RTOL, atol=ATOL, err_msg=f"{what}: against float64")
    if len(pairs):
        np.testing.assert_allclose(got, ref[pb * k + pi], rtol=RTOL, atol=ATOL, err_msg=f"{what}: survivors against float64")
    # no logit written past the count (per sub-batch): the other weights' logits are still there, and they are not the
    # standard weights' (the check would be empty if the two agreed)
    past = lst < 0 if fill else np.zeros(B * k, bool)
    if fill:
        np.testing.assert_array_equal(ex_on["logits"][past].view(np.uint32), before["logits"][past].view(np.uint32),
                                      err_msg=f"{what}: logits past the survivor count")
    if past.any():
        assert (before["logits"][past].view(np.uint32) != ex_off["logits"][past].view(np.uint32)).mean() > 0.9, what
    assert rows_on == rows_off, f"{what}: result rows with and without pruning"
    return rows_on, ex_on


# --------------------------------------------------------------------------------------------------------------- tests
def test_pool_gives_the_survivors_the_compositions_assume(pair):
    """An empty frame: every candidate survives; a leaf frame: candidate 0 alone; with top_k = 1 nobody."""
    import leafgrasp_amd as L

    for size, ks in ((BIG, (2, 20, 64)), (SMALL, (2, 3))):
        pool = _pool(size)
        pair[1].set_camera_params(pool.P)
        for k in ks:
            cands = pool.candidates(pair[1], k)
            for s, (xs, ys, tr) in enumerate(cands):
                assert len(xs) == k, (size, k, s, len(xs))
                keep = _survivors(xs, ys, tr, *size)
                assert keep == ([0] if s < pool.n_leaf else list(range(k))), (size, k, s, keep)
                if s < pool.n_leaf:   # not a near miss that float32 planes could turn: the runner-up's bound is far from trad 0
                    ub = tr[1:] + 0.3 * (1.0 - tr[1:]) ** 2
                    assert float(np.min(tr[0] - np.where(tr[1:] >= 0.5, ub, 0.7 * tr[1:] + 0.225))) > 0.01
                    assert not L._lib.lib.lg_cnn_candidate_cannot_win(float(tr[0]), float(tr[0]))


def test_every_device_plan(pair, num_cu):
    """Every batch of cnn_plan.prune_batches at the device's CU count that stays inside one slice."""
    layers = C.model_layers(STANDARD)
    batches = C.prune_batches(layers, num_cu)
    print()
    print(C.device_table(layers, batches, num_cu))
    pool = _pool(BIG)
    for name, B, k, e in batches:
        if B * k > C.MAX_SLICE:
            continue
        _check(pair, pool, _spread(B, e), k, name, target=C.survivors_of(B, k, e))


@pytest.mark.parametrize("name", [n for n, b, k, _ in C.EXTRA_BATCHES if b * k > C.MAX_SLICE])
def test_across_slices(pair, name):
    """More than 8192 patch slots: the pruned pass launches both slices and each takes its share of the device's count --
    8192 (the second slice runs on nothing), 8193 (on one patch), 8301 (on 109: no multiple of a tile block)."""
    _, B, k, e = next(t for t in C.EXTRA_BATCHES if t[0] == name)
    _, ex = _check(pair, _pool(BIG), _spread(B, e), k, name, target=int(name))
    assert B * k > C.MAX_SLICE and ex["counts"].tolist() == [int(name)]


def test_more_than_1024_frames(pair):
    """1030 frames of 96 x 128 at top_k = 3: lg_survivors_kernel's second round (frames 1024 ..) starts from the first
    round's total; both rounds hold empty and leaf frames."""
    B, k = 1030, 3
    is_empty = np.arange(B) % 3 == 1
    assert is_empty[1024:].any() and (~is_empty[1024:]).any() and is_empty[:1024].any() and (~is_empty[:1024]).any()
    e = int(is_empty.sum())
    _check(pair, _pool(SMALL), is_empty, k, "1030 frames", target=e * k + (B - e))


def test_small_call_after_a_large_one(pair):
    """8301 survivors, then 3 frames, then a call without survivors on ONE handle: each of the later calls gives what a fresh
    handle gives -- the slots past the new count still hold the earlier call's logits and nothing may read them.
    The calls follow each other directly (fill=False), so the past-the-count check of _check is made here against the handle's
    own previous export.  A stale logit that the rescoring did read would show in the rows: the candidates of an empty frame
    tie on the traditional score, so the winner and best_score of such a frame are decided by the logits alone."""
    pool = _pool(BIG)
    on = _handles([{}])[0]
    try:
        _, prev = _check(pair, pool, _spread(416, 415), 20, "8301 first", target=8301, on=on, fill=False)
        for what, B, k, e, target in (("3 frames after 8301", 3, 20, 1, 22), ("no survivor after that", 3, 1, 1, 0)):
            fresh = _handles([{}])[0]
            try:
                rows, ex = _check(pair, pool, _spread(B, e), k, what, target=target, on=on, fill=False)
                rows_f, ex_f = _check(pair, pool, _spread(B, e), k, what + " (fresh handle)", target=target, on=fresh, fill=False)
            finally:
                fresh.clear_cnn()
            assert rows == rows_f, what
            for f in ("counts", "list", "slot"):
                np.testing.assert_array_equal(ex[f], ex_f[f], err_msg=f"{what}: {f}")
            n = int(ex["counts"][0])
            np.testing.assert_array_equal(ex["logits"][:n].view(np.uint32), ex_f["logits"][:n].view(np.uint32), err_msg=what)
            # past the count the buffer still holds what the call before left there, and that is not what this call's
            # patches would give
            np.testing.assert_array_equal(ex["logits"][n:].view(np.uint32), prev["logits"][n:B * k].view(np.uint32),
                                          err_msg=f"{what}: logits past the survivor count")
            prev = ex
    finally:
        on.clear_cnn()


def test_sub_batches(pair):
    """LG_SUBBATCH=3 on 8 frames: sub-batches of 3, 3 and 2 frames with empty frames in the second and the third; each has its
    own count, list and logits (lg_ml_rescore's slot offset), and the rows are the one-sub-batch handle's."""
    pool = _pool(BIG)
    sub = _handles([{"LG_SUBBATCH": "3"}])[0]
    try:
        is_empty = np.array([0, 0, 0, 0, 1, 0, 1, 1], bool)
        rows, ex = _check(pair, pool, is_empty, 20, "LG_SUBBATCH=3", target=65, on=sub)
        assert (ex["sub_frames"], ex["n_sub"], ex["counts"].tolist()) == (3, 3, [3, 22, 40])
        rows1, ex1 = _check(pair, pool, is_empty, 20, "one sub-batch", target=65)
        assert rows == rows1 and ex1["counts"].tolist() == [65]
    finally:
        sub.clear_cnn()


# ------------------------------------------------------------------------------------ weights with which the CNN decides
DECIDING_SEEDS = (3, 4, 6, 9, 11, 12)


def test_cnn_decides_the_winner(pair):
    """The closed-form weights give ML scores within 0.005 of each other: the rescoring then hardly ever moves the winner and
    rows that are equal with and without pruning say little about logits.  Here the last layer is rescaled so that logit' =
    a (logit - med), med and a = 1.5 / std from the float64 logits of the test's own candidates, and the four score weights are
    halved (traditional scores below 0.5, where a candidate within 0.225 of the best survives): the winner is then often not
    candidate 0.  Pruned rows equal unpruned rows; the winner is the oracle's (float64 network) wherever the oracle's two best
    combined scores lie further apart than a logit error at tolerance can move them; ml_used is set where it must be."""
    from leafgrasp_amd.grasp_point_selector import _RESULT_DTYPE

    on, off = pair
    H, W, k = 384, 512, 20
    scenes = [O.synthetic_scene(H, W, s) for s in DECIDING_SEEDS]
    masks = np.stack([_largest_leaf(lab) for lab, _, _ in scenes]).astype(np.uint8)
    depths = np.stack([dep for _, dep, _ in scenes])
    P = scenes[0][2]
    m, d = torch.from_numpy(masks).cuda(), torch.from_numpy(depths).cuda()
    base = O.cnn_closed_form_params(seed=0)
    keep = {w: getattr(on.params, w) for w in WEIGHTS}
    try:
        for s in pair:
            s.set_camera_params(P)
            for w in WEIGHTS:
                setattr(s.params, w, keep[w] * 0.5)
        halved = {w: float(getattr(on.params, w)) for w in WEIGHTS}
        # the candidates and their dense patches, under the halved weights
        _, cands = off.select_grasp_candidates_batch(m, d, top_k=k)
        xy, patches = [], []
        for b in range(len(scenes)):
            rows = cands[b][cands[b]["index"] >= 0]
            rows = rows[np.argsort(rows["index"], kind="stable")]
            pts = [(int(x), int(y)) for x, y in zip(rows["x"], rows["y"])]
            maps = off.score_maps(m[b], d[b])[0]
            xy.append(pts)
            patches.append(off.gather_patches(m[b], d[b], maps, pts).cpu().numpy())
        l0 = np.concatenate([O.cnn_forward(base, p, dtype=torch.float64) for p in patches])
        med, std = float(np.median(l0)), float(np.std(l0))
        a = 1.5 / std
        deciding = dict(base)
        deciding["classifier.12.weight"] = (base["classifier.12.weight"].astype(np.float64) * a).astype(np.float32)
        deciding["classifier.12.bias"] = ((base["classifier.12.bias"].astype(np.float64) - med) * a).astype(np.float32)
        ref = [O.cnn_forward(deciding, p, dtype=torch.float64) for p in patches]
        print(f"\nbase logits: median {med:.4f} std {std:.4f}; a = {a:.2f}; rescaled logits {np.concatenate(ref).min():.2f} .. "
              f"{np.concatenate(ref).max():.2f}")
        for s in pair:
            s.set_cnn_state_dict(deciding)
        got = {}
        for name, s in (("pruned", on), ("all", off)):
            s.params.top_k = k
            s.select_grasp_points_batch(m, d)
            rows = bytes(s.last_results)
            res = np.frombuffer(rows, dtype=_RESULT_DTYPE).copy()
            ex = s.cnn_survivors()
            s.select_grasp_points_batch(m, d)
            assert bytes(s.last_results) == rows, f"{name}: repeated call"
            got[name] = (rows, res, ex)
        assert got["pruned"][0] == got["all"][0], "result rows with and without pruning"
        res, ex_on, ex_off = got["pruned"][1], got["pruned"][2], got["all"][2]
        # every logit of the unpruned pass against float64; every survivor's bit-equal to it
        for b in range(len(scenes)):
            n = len(xy[b])
            lo = ex_off["logits"][b * k:b * k + n]
            err = np.abs(lo - ref[b]) / (ATOL + RTOL * np.abs(ref[b]))
            worst["err"] = max(worst["err"], float(err.max()))
            np.testing.assert_allclose(lo, ref[b], rtol=RTOL, atol=ATOL, err_msg=f"frame {b} against float64")
            sl = ex_on["slot"][b * k:b * k + n]
            assert sl[0] >= 0
            np.testing.assert_array_equal(ex_on["logits"][sl[sl >= 0]].view(np.uint32), lo[sl >= 0].view(np.uint32))
        surv = [int((ex_on["slot"][b * k:(b + 1) * k] >= 0).sum()) for b in range(len(scenes))]
        # the oracle: float64 network on its own patches
        thr = 2 * 0.6 * a * 1e-4      # |d combined / d logit| <= 0.6 (w <= 0.3 ... ) times twice the logit tolerance, scaled by a
        ora = O.RefGraspPointSelector(cnn=lambda x: O.cnn_forward(deciding, x, dtype=torch.float64),
                                      params=O.ref_params(top_k=k, mask_is_bool=0, **halved))
        ora.set_camera_params(P)
        compared, moved_off_0, winners = 0, 0, []
        for b in range(len(scenes)):
            (best, _, _), dbg = ora.select_grasp_point(masks[b], depths[b], return_debug=True)
            oc = dbg["candidates"]
            assert oc == xy[b], f"frame {b}: candidates"
            trad = [float(dbg["scores"]["traditional_score"][y, x]) for x, y in oc]
            comb = []
            for t, ml in zip(trad, dbg["ml_scores"]):
                w = min(0.3, (1.0 - abs(ml - 0.5) * 2) * 0.6)
                comb.append((1.0 - w) * t + w * ml)
            vals = np.sort(np.array([trad[0]] + comb))
            gap = float(vals[-1] - vals[-2])
            win = oc.index(best)
            winners.append(win)
            print(f"frame {b} (seed {DECIDING_SEEDS[b]}): oracle winner candidate {win}, gap {gap:.2e} (threshold {thr:.2e}), "
                  f"ML scores {min(dbg['ml_scores']):.3f} .. {max(dbg['ml_scores']):.3f}, survivors {surv[b]}, "
                  f"device winner {(int(res['x'][b]), int(res['y'][b]))} ml_used {int(res['ml_used'][b])}")
            if gap <= thr:
                continue
            compared += 1
            moved_off_0 += win != 0
            assert (int(res["x"][b]), int(res["y"][b])) == best, f"frame {b}: winner"
            if win != 0:
                assert int(res["ml_used"][b]) == 1, f"frame {b}: ml_used"
        # conditions on the oracle alone: the comparison is not vacuous
        assert len(scenes) - compared <= len(scenes) // 4, (compared, winners)
        assert 3 * moved_off_0 >= compared, (moved_off_0, compared, winners)
    finally:
        for s in pair:
            s.params.top_k = 20
            for w in WEIGHTS:
                setattr(s.params, w, keep[w])
            s.set_cnn_state_dict(O.cnn_closed_form_params(seed=0))
