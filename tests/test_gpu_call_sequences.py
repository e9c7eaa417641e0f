"""One handle walked through the modes a node, a collector and a trainer sharing a selector put it through (-m gpu).

After EVERY step the bytes of everything the call returned must equal the bytes of the same step on a handle created for it
alone (tests/handle_cases.py: run_step, expected) -- history independence is exact: inside lg_select_grasp* no CNN item is
split, the candidate lists carry no atomics and the maxima are integers; lg_cnn_forward's split items add their parts in a fixed
order (lg_wino4_kernel: the owner adds the parts k = 1 .. P - 1 in turn), so its logits are held to bytes as well.  What stale
state could change is listed in DESIGN.md 1; tests/test_handle_cases_host.py holds the conditions under which it would show.

Independently of history the fresh-handle answers themselves are held to the oracle once per scene, at the tolerances the suite
already uses (RTOL / ATOL of test_gpu_parity.py for planes, 1e-5 for 3-D points, 1e-4 for logits)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import handle_cases as HC  # noqa: E402
from tests import label_aware_ref as R  # noqa: E402
from tests.handle_cases import S  # noqa: E402

RTOL, ATOL = 1e-4, 1e-6   # tests/test_gpu_parity.py
WALK_SEED, WALK_STEPS = 20261020, 40
SET_NAMES = list(HC.SETS)


def _sequences(w):
    sel = lambda *sc, **o: S("select", w, sc, **o)   # noqa: E731
    return {
        "1 sparse first": ((), [sel("A"), sel("B", dense=1), sel("C"), sel("A", dense=1)]),
        "2 dense first": ((), [sel("A", dense=1), sel("B"), sel("C", dense=1), sel("A"), sel("B"), sel("empty"), sel("full"),
                               sel("empty", dense=1), sel("full", dense=1), sel("B")]),
        "3 CNN on, off, swapped": ((), [sel("D"), S("set_cnn", w, seed=0), sel("D"), S("cands", w, ("D",), k=20), sel("D"),
                                        S("clear_cnn", w), sel("D"), S("set_cnn", w, seed=1), sel("D"), S("load_trainer", w, seed=0),
                                        sel("D"), S("cnn_forward", w, n=HC.SPLIT_N), sel("A"), S("cnn_forward", w, n=1), sel("D")]),
        "4 labels": ((), [S("set_cnn", w, seed=0), S("leaves", w, ("A",), la=0), S("leaves", w, ("A",), la=1),
                          S("leaves", w, ("C",), la=1), sel("A"), S("leaves", w, ("B",), la=1), S("leaves", w, ("B", "C", "A"), la=1),
                          S("leaves", w, ("A",), la=1, id=7), S("refused", w, ("A",), kind="la_mask"), S("leaves", w, ("A",), la=0),
                          S("cands_leaves", w, ("A",), la=1), S("cands_leaves", w, ("A",), la=0)]),
        "5 sizes": ((), [S("set_cnn", w, seed=0), sel("A", "B", "C"), sel("C", "empty", "A", "D", "B", "full", "A"), sel("B"),
                         sel("A", "B", "C"), S("cands", w, ("D", "B", "C"), k=20), S("cands", w, ("D", "B", "C"), k=64),
                         S("cands", w, ("D", "B", "C"), k=1), S("cands", w, ("D", "B", "C"), k=20), sel("B", g=7),
                         S("refused", w, ("A",), kind="g9"), sel("B", g=1), sel("B"), sel("D", bool=1), sel("D"), sel("D", bool=1),
                         sel("A", bool=1), sel("A")]),
        "6 foreign entries between selects": ((), [S("set_cnn", w, seed=0), sel("A"), S("topk", w, ("B",)), sel("B"), S("orient", w),
                                                   sel("A"), S("midrib", w), sel("B"), S("negmasks", w, ("B",)), sel("A"),
                                                   S("evaluate", w), sel("B"), S("harvest", w, ("C",)), sel("A"),
                                                   S("gather", w, ("C",)), sel("B"), S("score_maps", w, ("C", "B")), sel("A"),
                                                   S("refused", w, ("A",), kind="pcl"), sel("B")]),
        "7 orientation hand-back, small scratch": ((("LG_ORIENT_CAP", HC.ORIENT_CAP),),
                                                    [sel("over"), sel("A"), sel("over", "A", "over"), sel("A", dense=1), sel("over", dense=1)]),
        "7 orientation hand-back, host analysis": ((("LG_HOST_ORIENT", 1),),
                                                    [sel("over"), sel("A"), sel("over", "A", "over"), sel("A", dense=1), sel("over", dense=1)]),
    }


SEQUENCES = {f"{t} @ {w}": v for w in SET_NAMES for t, v in _sequences(w).items()}


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available()


@pytest.mark.parametrize("title", list(SEQUENCES))
def test_scripted_sequence(title):
    env, steps = SEQUENCES[title]
    hd = HC.Handle(steps[0][1], env)
    got = HC.walk(hd, steps, note=title + ": ")
    by = dict(zip(range(len(steps)), got))
    if title.startswith("3 "):
        none, s0, s0_again, cleared, s1, from_trainer = by[0], by[2], by[4], by[6], by[8], by[10]
        assert s0 == s0_again == from_trainer, "the candidates entry and load_from_trainer leave the seed-0 answer alone"
        assert cleared == none, "clear_cnn gives the answer of a handle without a model"
        assert len({none, s0, s1}) == 3, "D's answer moves with the model: a stale model would show"
        assert by[14] == s0
    if title.startswith("4 "):
        assert by[1] != by[2], "the label-aware rows of A differ from the default ones (pre-grasp or CNN channel 5)"
    if title.startswith("5 "):
        assert by[13] != by[14], "a bool mask leaves D's border candidates unscored: its rows differ from the uint8 mask's"


@pytest.mark.parametrize("set_", SET_NAMES)
def test_sparse_calls_hold_three_planes_until_a_dense_one(set_):
    """sequence 1 with the workspace in view: a handle with a model that has only made sparse calls holds three planes of its
    own (without a model: two); the dense call adds the rest and the sparse calls after it still give their fresh-handle bytes"""
    hd = HC.Handle(set_)
    HC.walk(hd, [S("select", set_, ("A",))])
    assert {n for n, b in hd.sel.ws_plane_bytes().items() if b} == {"distance_map", "traditional_score"}
    hd = HC.Handle(set_, model="seed0")
    HC.walk(hd, [S("select", set_, ("A",))])
    held = {n for n, b in hd.sel.ws_plane_bytes().items() if b}
    assert held == {"distance_map", "traditional_score", "flatness_map"}, held
    HC.walk(hd, [S("select", set_, ("B",), dense=1)])
    assert {n for n, b in hd.sel.ws_plane_bytes().items() if b} >= held   # (the dense call writes the caller's planes)
    HC.walk(hd, [S("select", set_, ("C",)), S("select", set_, ("A",), dense=1), S("select", set_, ("B",))])


@pytest.mark.parametrize("set_", SET_NAMES)
def test_the_small_scratch_hands_the_speckled_frame_back(set_):
    """sequence 7's premise on the device: with LG_ORIENT_CAP=64 the speckled frame is analysed on the host (redo count 1, then 2
    of the mixed batch), A is not"""
    from leafgrasp_amd._lib import lib
    import ctypes as C

    hd = HC.Handle(set_, (("LG_ORIENT_CAP", HC.ORIENT_CAP),))
    assert lib.lg_orientation_note(hd.sel._h) == b""
    n = C.c_int32(-1)
    for names, want in ((("over",), 1), (("A",), 0), (("over", "A", "over"), 2)):
        HC.walk(hd, [S("select", set_, names)])
        assert lib.lg_debug_orient_redo(hd.sel._h, C.byref(n)) == 0 and n.value == want, (names, n.value)


@pytest.mark.parametrize("set_", SET_NAMES)
def test_random_walk(set_):
    vocab = HC.vocabulary(set_)
    rng = np.random.default_rng(WALK_SEED + SET_NAMES.index(set_))
    steps = [vocab[int(i)] for i in rng.integers(0, len(vocab), WALK_STEPS)]
    assert len({s[0] for s in steps}) >= 8
    HC.walk(HC.Handle(set_), steps, note=f"walk seed {WALK_SEED} @ {set_}: ")


# ------------------------------------------------------------------------------------------- the fresh handle and the oracle
def _rows(sel):
    from leafgrasp_amd.grasp_point_selector import _RESULT_DTYPE
    return np.frombuffer(bytes(sel.last_results), dtype=_RESULT_DTYPE)


def _ref(set_, seed=None, labels=None):
    cnn = None if seed is None else (lambda x, p=HC.cnn_params(seed): O.cnn_forward(p, x))
    ref = O.RefGraspPointSelector(cnn=cnn) if labels is None else R.LabelAwareRef(labels, 1, cnn=cnn)
    ref.set_camera_params(HC.P_of(set_))
    return ref


def _check_row(row, exp, what):
    (xy, g3, pre) = exp
    assert row["found"] == 1 and (int(row["x"]), int(row["y"])) == xy, (what, row, xy)
    np.testing.assert_allclose([row["X"], row["Y"], row["Z"]], g3, rtol=1e-5, err_msg=what)
    assert bool(row["has_pre"]) == (pre is not None), what
    if pre is not None:
        np.testing.assert_allclose([row["pX"], row["pY"], row["pZ"]], pre, rtol=1e-5, err_msg=what)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "full", "over"])
@pytest.mark.parametrize("set_", SET_NAMES)
def test_fresh_handle_select_and_candidates_against_the_oracle(set_, name):
    lab, dep = HC.scene(set_, name)
    m = (lab == 1).astype(np.uint8)
    for seed in (None, 0) if name in "ABCD" else (None,):
        hd = HC.Handle(set_, model="none" if seed is None else f"seed{seed}")
        exp, dbg = _ref(set_, seed).select_grasp_point(m, dep, mask_is_bool=False, return_debug=True)
        for dense in (0, 1):
            HC.run_step(hd, S("select", set_, (name,), dense=dense))
            _check_row(_rows(hd.sel)[0], exp, f"select {name} seed {seed} dense {dense}")
        _, c = hd.sel.select_grasp_candidates_batch(torch.from_numpy(m).cuda(), torch.from_numpy(dep).cuda())
        rows = [r for r in c[0] if r["index"] >= 0]
        assert sorted((int(r["x"]), int(r["y"])) for r in rows) == sorted(dbg["candidates"]), name
        assert (int(rows[0]["x"]), int(rows[0]["y"])) == exp[0]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "full", "over"])
@pytest.mark.parametrize("set_", SET_NAMES)
def test_fresh_handle_planes_against_the_oracle(set_, name):
    from leafgrasp_amd._lib import MAP_NAMES

    lab, dep = HC.scene(set_, name)
    m = (lab == 1).astype(np.uint8)
    hd = HC.Handle(set_)
    maps, valid, _ = hd.sel.score_maps(torch.from_numpy(m).cuda(), torch.from_numpy(dep).cuda())
    ref = _ref(set_)
    sc = ref._calculate_all_scores(m, dep)
    for k in MAP_NAMES:
        np.testing.assert_allclose(maps[k].cpu().numpy(), sc[k], rtol=RTOL, atol=ATOL, err_msg=f"{name} {k}")
    assert np.array_equal(valid.cpu().numpy() != 0, ref._get_valid_regions(m, sc)), name


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("set_", SET_NAMES)
def test_fresh_handle_label_aware_against_the_reference(set_, name):
    lab, dep = HC.scene(set_, name)
    for seed in (None, 0):
        hd = HC.Handle(set_, model="none" if seed is None else f"seed{seed}")
        HC.run_step(hd, S("leaves", set_, (name,), la=1))
        ref = _ref(set_, seed, labels=lab)
        _check_row(_rows(hd.sel)[0], ref.select(dep, mask_is_bool=True), f"leaves {name} seed {seed}")


@pytest.mark.parametrize("n", [1, HC.SPLIT_N])
def test_fresh_handle_logits_against_the_oracle(n):
    hd = HC.Handle("wide", model="seed0")
    got = np.frombuffer(HC.run_step(hd, S("cnn_forward", "wide", n=n)), np.float32)
    np.testing.assert_allclose(got, O.cnn_forward(HC.cnn_params(0), HC.patches_of(n)), rtol=1e-4, atol=1e-4)
