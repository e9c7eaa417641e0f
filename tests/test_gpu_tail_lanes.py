"""The tail lanes of lg_select_grasp ("Tail in lanes") against the one-lane call.

Behind the front the batch is cut into lanes of consecutive frames; every lane runs planes -> top-k -> survivors -> gather ->
CNN on a stream of its own, beside the other lanes.  No kernel's arithmetic changes, so a call in lanes must give what the
one-lane call gives bit for bit: the result rows, the number of patches scored and, survivor by survivor, the logit.  What
could go wrong is the plumbing -- the range of the near-tile list a lane's plane launch takes, its survivor list, count and
slot map, its range of the CNN's activation buffers, the order of the streams -- and the compositions below aim at each.

Frames are 160 x 224 (3.5 tiles wide) or 104 x 264 (6.5 tile rows) windows of the synthetic scenes, from the pool of
tests/test_gpu_cnn_prune_regimes.py: a leaf frame keeps few candidates, an empty mask keeps them all, and the scenes differ, so
a patch, count or activation taken from a neighbouring frame or lane shows.  Lanes are forced through lg_debug_tail_lanes
(GraspPointSelector.tail_lanes), on handles of their own."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import cnn_plan as CP  # noqa: E402
from tests import test_gpu_cnn_prune_regimes as R  # noqa: E402
from tests.test_gpu_cnn_regimes import ATOL, RTOL  # noqa: E402

SIZE, SIZE_PARTIAL_ROWS = (160, 224), (104, 264)
WEIGHTS = R.WEIGHTS


@pytest.fixture(scope="module")
def lane_handles():
    """{lanes: a selector of its own with that many lanes forced}"""
    assert torch.cuda.is_available()
    hs = dict(zip((1, 2, 3, 4), R._handles([{}] * 4)))
    for n, s in hs.items():
        s.tail_lanes(n)
    yield hs
    for s in hs.values():
        s.clear_cnn()


def _fresh(lanes):
    s = R._handles([{}])[0]
    s.tail_lanes(lanes)
    return s


def _plan(B, lanes):
    n, sb = C.c_int32(), C.c_int32()
    from leafgrasp_amd._lib import lib

    assert lib.lg_tail_lane_plan(B, lanes, 1, C.byref(n), C.byref(sb)) == 0
    return int(n.value), int(sb.value)


def _near_off(sel, B):
    """first entry of every frame in the near-tile list of the selector's last call, [B + 1] (lg_debug_near_tiles)"""
    from leafgrasp_amd._lib import lib

    off = (C.c_int32 * (B + 1))()
    assert lib.lg_debug_near_tiles(sel._h, off, B + 1) == 0
    return list(off)


def _run(sel, pool, m, d, k):
    """-> (result rows as bytes, patches scored, {(frame, candidate): logit bits} of the survivors, export, lanes the call ran in)"""
    sel.set_camera_params(pool.P)
    sel.params.top_k = k
    try:
        sel.select_grasp_points_batch(m, d)
        rows, scored, ex, ran = bytes(sel.last_results), sel.cnn_scored(), sel.cnn_survivors(), sel.tail_lanes()
    finally:
        sel.params.top_k = 20
    B, sb, logits = m.shape[0], ex["sub_frames"], {}
    for s, count in enumerate(ex["counts"].tolist()):
        off = s * sb
        n = min(sb, B - off)
        assert 0 <= count <= n * k
        for j in range(count):
            e = int(ex["list"][off * k + j])
            assert 0 <= e < n * k and int(ex["slot"][(off + e // k) * k + e % k]) == j
            key = (off + e // k, e % k)
            assert key not in logits
            logits[key] = int(ex["logits"][off * k + j:off * k + j + 1].view(np.uint32)[0])
    assert scored == len(logits) == int(ex["counts"].sum())
    return rows, scored, logits, ex, ran


def _same(hs, pool, m, d, k, lanes, what):
    """The call on the handles of `lanes` against the one-lane handle's; -> the one-lane call's (rows, scored, logits, export)."""
    B = m.shape[0]
    one = _run(hs[1], pool, m, d, k)
    assert one[4] == 1 and (one[3]["n_sub"], one[3]["sub_frames"]) == (1, B), what
    for n in lanes:
        got = _run(hs[n], pool, m, d, k)
        want_lanes, sb = _plan(B, n)
        assert got[4] == want_lanes and (got[3]["n_sub"], got[3]["sub_frames"]) == (want_lanes, sb), (what, n, got[4], want_lanes)
        assert got[0] == one[0], f"{what}: result rows, {n} lanes against one"
        assert got[1] == one[1], f"{what}: patches scored, {n} lanes against one"
        assert got[2] == one[2], f"{what}: survivors and their logit bits, {n} lanes against one"
    return one


def _mixed(B):
    """leaf and empty frames in turn, a leaf frame first; the scenes cycle through the pool's"""
    return np.arange(B) % 2 == 1


# -------------------------------------------------------------------------------------------------------- lanes against one lane
def _deciding_params(sel, pool, k):
    """The closed-form weights with the last layer rescaled as test_cnn_decides_the_winner does -- logit' = a (logit - med), a =
    1.5 / std -- here from the device's own logits of the pool's scenes: only the spread matters, the comparison is lane
    against lane."""
    base = O.cnn_closed_form_params(seed=0)
    sel.set_cnn_state_dict(base)
    sel.set_camera_params(pool.P)
    sel.select_grasp_candidates_batch(pool.masks, pool.depths, top_k=k)
    l0 = sel.cnn_survivors()["logits"].astype(np.float64)
    med, a = float(np.median(l0)), 1.5 / float(np.std(l0))
    out = dict(base)
    out["classifier.12.weight"] = (base["classifier.12.weight"].astype(np.float64) * a).astype(np.float32)
    out["classifier.12.bias"] = ((base["classifier.12.bias"].astype(np.float64) - med) * a).astype(np.float32)
    return out


@pytest.mark.parametrize("weights", ("standard", "deciding"))
def test_lanes_against_one_lane(lane_handles, weights):
    """2, 3 and 4 lanes against one at B = 1 (the lanes clamp to one), 2, 4, 5 (3 + 2 in two lanes) and 7 (3 + 3 + 1 in three):
    rows, patches scored, and every survivor's logit bits."""
    from leafgrasp_amd.grasp_point_selector import _RESULT_DTYPE

    hs, pool, k = lane_handles, R._pool(SIZE), 20
    keep = {w: getattr(hs[1].params, w) for w in WEIGHTS}
    assert _plan(1, 4) == (1, 1) and _plan(5, 2) == (2, 3) and _plan(7, 3) == (3, 3)
    try:
        if weights == "deciding":   # halved score weights: more candidates stay in reach of the best, and the logits decide
            for s in hs.values():
                for w in WEIGHTS:
                    setattr(s.params, w, keep[w] * 0.5)
            params = _deciding_params(hs[1], pool, k)
            for s in hs.values():
                s.set_cnn_state_dict(params)
        by_ml = frames = 0
        for B in (1, 2, 4, 5, 7):
            m, d = pool.frames(pool.scene_ids(_mixed(B)))
            one = _same(hs, pool, m, d, k, (2, 3, 4), f"{weights}, B = {B}")
            res = np.frombuffer(one[0], dtype=_RESULT_DTYPE)
            by_ml += int(res["ml_used"].sum())
            frames += B
            print(f"{weights}: B {B}: {one[1]} of {B * k} patches scored, ml_used in {int(res['ml_used'].sum())} frames")
        print(f"{weights}: the CNN decided {by_ml} of {frames} frames")
        if weights == "deciding":
            assert by_ml > 0, "the rescaled last layer must let the CNN decide some frame, or the rows say little about logits"
    finally:
        for s in hs.values():
            for w in WEIGHTS:
                setattr(s.params, w, keep[w])
            s.set_cnn_state_dict(O.cnn_closed_form_params(seed=0))


# ------------------------------------------------------------------------------------- compositions that empty a lane's work
def test_a_lane_of_empty_masks(lane_handles):
    """Two lanes of two frames; lane 1, then lane 0, holds empty masks only: every candidate of it survives, and its range of
    the near-tile list is empty (the plane launch of that lane launches nothing)."""
    hs, pool, k = lane_handles, R._pool(SIZE), 20
    for empty_lane in (1, 0):
        is_empty = np.zeros(4, bool)
        is_empty[2 * empty_lane:2 * empty_lane + 2] = True
        m, d = pool.frames(pool.scene_ids(is_empty))
        _same(hs, pool, m, d, k, (2,), f"lane {empty_lane} of empty masks")
        ex = hs[2].cnn_survivors()
        assert int(ex["counts"][empty_lane]) == 2 * k and 0 < int(ex["counts"][1 - empty_lane]) < 2 * k
        off = _near_off(hs[2], 4)
        assert off[2 * empty_lane + 2] == off[2 * empty_lane], "the empty lane owns no near tile"
        assert off[2 * (1 - empty_lane) + 2] > off[2 * (1 - empty_lane)]


def test_nobody_survives(lane_handles):
    """top_k = 1: a frame's only candidate needs no CNN; the count is 0 in every lane."""
    hs, pool = lane_handles, R._pool(SIZE)
    m, d = pool.frames(pool.scene_ids(_mixed(5)))
    _same(hs, pool, m, d, 1, (2, 3, 4), "top_k = 1")
    for n in (2, 3, 4):
        assert not hs[n].cnn_survivors()["counts"].any()


def test_nan_depth_pixel_on_the_leaf(lane_handles):
    """One frame of the second lane with a NaN depth pixel at the middle of its leaf."""
    hs, pool, k = lane_handles, R._pool(SIZE), 20
    m, d = pool.frames(pool.scene_ids(np.array([0, 1, 0, 0, 1], bool)))
    d = d.clone()
    ys, xs = np.nonzero(m[3].cpu().numpy())
    assert len(ys)
    d[3, int(np.median(ys)), int(np.median(xs))] = float("nan")
    _same(hs, pool, m, d, k, (2, 3), "NaN depth pixel")


@pytest.mark.parametrize("size", (SIZE, SIZE_PARTIAL_ROWS))
def test_bool_and_uint8_masks(lane_handles, size):
    """torch.bool masks take the border rule of the rescoring (fewer survivors near the frame's edge); uint8 masks do not."""
    hs, pool, k = lane_handles, R._pool(size), 20
    m, d = pool.frames(pool.scene_ids(_mixed(5)))
    scored = [_same(hs, pool, mm, d, k, (2, 3), f"{size} {mm.dtype}")[1] for mm in (m, m.bool())]
    print(f"{size}: patches scored with uint8 / bool masks: {scored}")


# ------------------------------------------------------------------------------------------------------------ activation ranges
@pytest.mark.parametrize("k", (20, 64))
def test_activation_ranges(lane_handles, k):
    """Lanes of 3 + 2 frames, every lane with survivors from leaf and empty frames of different scenes: the lanes' CNN passes run
    beside each other, each in its own range of every activation buffer.  Every survivor's logit is the one-lane call's bit for
    bit and lies within the project's tolerance of the float64 network on that candidate's own patch."""
    hs, pool = lane_handles, R._pool(SIZE)
    ids = pool.scene_ids(np.array([0, 1, 0, 1, 0], bool))
    m, d = pool.frames(ids)
    one = _same(hs, pool, m, d, k, (2,), f"activation ranges, top_k {k}")
    counts = hs[2].cnn_survivors()["counts"].tolist()
    assert len(counts) == 2 and min(counts) > k, counts
    params = O.cnn_closed_form_params(seed=0)
    hs[1].set_camera_params(pool.P)
    cands = pool.candidates(hs[1], k)
    two = _run(hs[2], pool, m, d, k)[2]
    worst = 0.0
    for b, s in enumerate(ids.tolist()):
        mine = sorted(c for f, c in two if f == b)
        xs, ys, _ = cands[s]
        ref = pool.ref_logits(hs[1], s, xs[mine], ys[mine], params)
        got = np.array([two[(b, c)] for c in mine], np.uint32).view(np.float32)
        worst = max(worst, float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max()))
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"frame {b} (scene {s}) against float64")
    print(f"top_k {k}: {len(two)} survivors in lanes {counts}, largest logit error {worst:.3f} of the tolerance")
    assert two == one[2]


# -------------------------------------------------------------------------------------------------- one handle across modes
def test_one_handle_across_modes():
    """lanes 2 -> lanes 1 -> candidates entry -> lanes 3 -> planes taken back -> lanes 2 on fewer frames, on ONE handle: each
    step gives what a fresh handle gives for that step alone, byte for byte."""
    pool, k = R._pool(SIZE), 20
    m7, d7 = pool.frames(pool.scene_ids(_mixed(7)))

    def step(sel, what):
        sel.set_camera_params(pool.P)
        kind, lanes, B = what
        m, d = m7[:B], d7[:B]
        if lanes is not None:
            sel.tail_lanes(lanes)
        if kind == "select":
            rows, scored, logits, _, ran = _run(sel, pool, m, d, k)
            assert ran == _plan(B, lanes)[0]
            return rows, scored, tuple(sorted(logits.items()))
        if kind == "candidates":
            _, cands = sel.select_grasp_candidates_batch(m, d, top_k=k)
            assert sel.tail_lanes() == 1, "the candidates entry stays one lane"
            return bytes(sel.last_results), cands.tobytes()
        _, maps, valid = sel.select_grasp_points_batch(m, d, return_maps=True)
        assert sel.tail_lanes() == 1, "a dense call stays one lane"
        return (bytes(sel.last_results), valid.cpu().numpy().tobytes()) + tuple(maps[n].cpu().numpy().tobytes() for n in sorted(maps))

    steps = (("select", 2, 7), ("select", 1, 7), ("candidates", None, 7), ("select", 3, 7), ("maps", None, 7), ("select", 2, 3))
    one = _fresh(0)
    try:
        for i, what in enumerate(steps):
            got = step(one, what)
            fresh = _fresh(0)
            try:
                assert got == step(fresh, what), f"step {i} {what}: the handle's history shows"
            finally:
                fresh.clear_cnn()
    finally:
        one.clear_cnn()


# ------------------------------------------------------------------------------------------------------------------ stream order
def test_stream_order(lane_handles):
    """A two-lane call behind a delay kernel on a caller stream of its own.  The inputs hold another scene until the delay has
    passed and again right behind the call, all in stream order and without a host wait in between: the lanes' library streams
    must start behind what the caller queued, and the caller's stream must go on only behind every lane.  The rows are the true
    scene's."""
    from tests.handle_cases import sleep_cycles_per_ms

    hs, pool, k = lane_handles, R._pool(SIZE), 20
    sel = hs[2]
    true = pool.frames(pool.scene_ids(_mixed(4)))
    decoy = pool.frames(pool.scene_ids(~_mixed(4)))
    want, want_decoy = _run(hs[1], pool, *true, k)[0], _run(hs[1], pool, *decoy, k)[0]
    assert want != want_decoy
    _run(sel, pool, *true, k)   # (the workspace of this shape exists from here on)
    m, d = decoy[0].clone(), decoy[1].clone()
    cycles = sleep_cycles_per_ms()
    stream, ev = torch.cuda.Stream(), torch.cuda.Event()
    torch.cuda.synchronize()
    sel.set_camera_params(pool.P)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(20 * cycles))
        ev.record(stream)
        m.copy_(true[0], non_blocking=True)
        d.copy_(true[1], non_blocking=True)
        sel.select_grasp_points_batch(m, d)
        rows = bytes(sel.last_results)
        m.copy_(decoy[0], non_blocking=True)
        d.copy_(decoy[1], non_blocking=True)
    torch.cuda.synchronize()
    assert sel.tail_lanes() == 2
    assert rows != want_decoy, "the call read its inputs before the caller's stream had written them"
    assert rows == want


# ---------------------------------------------------------------------------------------------------------------- profiling slots
def test_profiling_slots_count_one_launch_per_call(lane_handles):
    """lg_profile_enable(1), two lanes at B = 4: every slot of the launch table of profiles/NOTES_select_front.md
    (lg_select_grasp with a model) reads one launch -- lane 1's scopes add their time to the launch lane 0 counted."""
    from leafgrasp_amd._lib import lib

    pool, k = R._pool(SIZE), 20
    sel = _fresh(2)
    try:
        m, d = pool.frames(pool.scene_ids(_mixed(4)))
        _run(sel, pool, m, d, k)
        table = {}
        for mode, names in ((1, ("prep", "bbox", "orient", "stem", "dt_border", "dt_hrun", "dt_search", "dt_fwd", "dt_bwd", "final",
                                 "near_tiles", "topk", "finish", "survivors", "gather", "cnn")), (2, ("final",))):
            assert lib.lg_profile_enable(sel._h, mode) == 0
            _run(sel, pool, m, d, k)
            assert sel.tail_lanes() == 2
            torch.cuda.synchronize()
            for name in names:
                n, ms = C.c_int(0), C.c_double(0.0)
                lib.lg_profile_read(sel._h, name.encode(), C.byref(n), C.byref(ms))
                table[(mode, name)] = (n.value, ms.value)
        lib.lg_profile_enable(sel._h, 0)
        print({f"{mode}:{name}": v for (mode, name), v in table.items()})
        assert all(n == 1 for n, _ in table.values()), table
        assert all(ms > 0 for _, ms in table.values()), table
    finally:
        sel.clear_cnn()


# ------------------------------------------------------------------------------------------------------------------- LG_TRACE
def _trace_lines(err, B):
    """stderr of ONE traced call -> the four numbers of its `gpu timeline` line (None: the call printed none); the host line
    must be there once."""
    lines = err.splitlines()
    assert sum(ln.startswith(f"[lg] B={B} enq1 ") for ln in lines) == 1, err
    gpu = [ln for ln in lines if ln.startswith("[lg] gpu timeline")]
    assert len(gpu) <= 1, err
    if not gpu:
        return None
    _, _, fields = gpu[0].partition("):")
    names, nums = zip(*(f.strip().rsplit(" ", 1) for f in fields.split("|")))
    assert names == ("sweeps done", "planes", "topk", "cnn"), gpu[0]
    return [float(x) for x in nums]


def test_trace_lines_per_schedule(capfd):
    """Handles created under LG_TRACE=1, stderr captured at the file descriptor.  B = 4 forced to one lane, then to two: the rows
    are an untraced handle's byte for byte, and each call prints one host line and one device timeline whose four marks --
    sweeps, planes, top-k, CNN, all on lane 0's stream -- are finite, not negative and in order.  LG_SUBBATCH=2 at B = 5: the
    host line only (the stages run on the library's streams), rows equal to the one-sub-batch handle's."""
    pool, k = R._pool(SIZE), 20
    plain, traced, piped = R._handles([{}, {"LG_TRACE": "1"}, {"LG_TRACE": "1", "LG_SUBBATCH": "2"}])   # (a setting stays for the next)
    try:
        assert traced.options()["LG_TRACE"] == 1 and plain.options()["LG_TRACE"] == 0
        assert piped.options()["LG_TRACE"] == 1 and piped.options()["LG_SUBBATCH"] == 2
        m, d = pool.frames(pool.scene_ids(_mixed(4)))
        for lanes in (1, 2):
            plain.tail_lanes(lanes)
            traced.tail_lanes(lanes)
            want = _run(plain, pool, m, d, k)
            capfd.readouterr()
            got = _run(traced, pool, m, d, k)
            err = capfd.readouterr().err
            assert want[4] == got[4] == lanes
            assert got[0] == want[0], f"{lanes} lanes: a traced handle's rows against an untraced handle's"
            marks = _trace_lines(err, 4)
            print(f"{lanes} lanes: gpu timeline {marks}")
            assert marks is not None and len(marks) == 4 and all(np.isfinite(marks)), err
            assert marks[0] >= 0 and all(a <= b for a, b in zip(marks, marks[1:])), err
        m, d = pool.frames(pool.scene_ids(_mixed(5)))
        plain.tail_lanes(0)
        want = _run(plain, pool, m, d, k)
        capfd.readouterr()
        got = _run(piped, pool, m, d, k)
        err = capfd.readouterr().err
        assert (got[3]["n_sub"], got[3]["sub_frames"]) == (3, 2) and (want[3]["n_sub"], want[3]["sub_frames"]) == (1, 5)
        assert got[0] == want[0], "LG_SUBBATCH=2: rows against the one-sub-batch handle's"
        assert _trace_lines(err, 5) is None, err
    finally:
        for s in (traced, plain, piped):
            s.clear_cnn()


# --------------------------------------------------------------------------------------------------- the 8192-patch slice boundary
def test_second_slice_in_one_lane():
    """129 frames at top_k = 64 with 8193 survivors (tests/cnn_plan.py): once the automatic rule cuts a batch of this size into
    lanes no lane reaches the second 8192-patch slice of lg_cnn_run.  Forced to one lane the pruned pass still launches both
    slices, the second on one patch: everything test_gpu_cnn_prune_regimes.py holds such a call to."""
    _, B, k, e = next(t for t in CP.EXTRA_BATCHES if t[0] == "8193")
    on, off = R._handles([{}, {"LG_CNN_PRUNE": "0"}])
    on.tail_lanes(1)
    try:
        _, ex = R._check((on, off), R._pool(R.BIG), R._spread(B, e), k, "8193 in one lane", target=8193)
        assert on.tail_lanes() == 1 and B * k > CP.MAX_SLICE and ex["counts"].tolist() == [8193]
    finally:
        on.clear_cnn()
        off.clear_cnn()
