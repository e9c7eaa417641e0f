"""The conditions that make the handle tests (tests/test_gpu_call_sequences.py, tests/test_gpu_stream_order.py) able to fail,
checked on the scenes of tests/handle_cases.py with the oracle and the host exports alone:

  rescoring runs      every scene with a leaf has at least two candidates
  distinct answers    the picks of A, B and C differ pairwise (a stale row, tile or input shows as another scene's answer); D
                      has no valid pixel and its pick differs between no model, seed 0 and seed 1 (a stale model shows)
  stale tiles matter  each scene's rectangle of near tiles (lg_near_tile_rect, at the widest halo in use) is a strict subset of
                      the frame, and those of A and B are disjoint: B after A runs on tiles A never wrote, beside tiles A did
  labels matter       A and B have another leaf within 20 px of leaf 1, C has none, and the label-aware isolation plane of A
                      differs from the default one
  orientation         the speckled frame has more runs than the small scratch of sequence 7 holds, A has fewer
  scripts             every step of a scripted sequence and of the walk's vocabulary names an entry of the vocabulary"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402
from tests import handle_cases as HC  # noqa: E402
from tests import label_aware_ref as R  # noqa: E402
from tests import near_tiles_ref as NT  # noqa: E402

SET_NAMES = list(HC.SETS)
_memo = {}


def picked(set_, name, seed=None):
    """(pick, candidates) of the oracle on leaf 1 of a scene, uint8 mask, with the closed-form CNN of `seed` or without"""
    key = (set_, name, seed)
    if key not in _memo:
        lab, dep = HC.scene(set_, name)
        cnn = None if seed is None else (lambda x, p=HC.cnn_params(seed): O.cnn_forward(p, x))
        ref = O.RefGraspPointSelector(cnn=cnn)
        ref.set_camera_params(HC.P_of(set_))
        res, dbg = ref.select_grasp_point((lab == 1).astype(np.uint8), dep, mask_is_bool=False, return_debug=True)
        _memo[key] = (res[0], dbg.get("candidates", []), dbg)
    return _memo[key]


@pytest.mark.parametrize("set_", SET_NAMES)
def test_every_scene_with_a_leaf_has_candidates_to_rescore(set_):
    for name in ("A", "B", "C", "D", "full", "over"):
        pick, cands, _ = picked(set_, name)
        assert pick is not None and len(cands) >= 2, (name, len(cands))
    for name in ("A", "B", "C"):   # valid pixels exist: the pick lies on the leaf and scored above zero
        pick, _, dbg = picked(set_, name)
        assert dbg["valid"][pick[1], pick[0]], name
    assert not picked(set_, "D")[2]["valid"].any(), "D takes the zero-score fall-through"


@pytest.mark.parametrize("set_", SET_NAMES)
def test_picks_differ_between_scenes_and_between_models(set_):
    a, b, c = (picked(set_, n)[0] for n in "ABC")
    assert len({a, b, c}) == 3, (a, b, c)
    d = [picked(set_, "D", seed)[0] for seed in (None, 0, 1)]
    print(set_, "A, B, C:", a, b, c, "D without / seed 0 / seed 1:", d)
    assert len(set(d)) == 3, d


def near_rect(set_, name, halo=4):
    H, W = HC.shape_of(set_)
    box = NT.bbox(HC.scene(set_, name)[0] == 1)
    rect = (C.c_int32 * 4)()
    n = _lib.lib.lg_near_tile_rect(box[0], box[1], box[2], box[3], H, W, halo, rect)
    return tuple(rect), n


@pytest.mark.parametrize("set_", SET_NAMES)
def test_near_tiles_are_a_strict_subset_and_those_of_a_and_b_are_disjoint(set_):
    H, W = HC.shape_of(set_)
    tiles_x, tiles_y = NT.tile_grid(H, W)
    rects = {}
    for name in ("A", "B", "C", "D", "over"):
        rects[name], n = near_rect(set_, name)
        if name != "over":   # (the specks of "over" lie everywhere)
            assert 0 < n < tiles_x * tiles_y, (name, rects[name])
    (ax0, ax1, ay0, ay1), (bx0, bx1, by0, by1) = rects["A"], rects["B"]
    assert ax1 < bx0 or bx1 < ax0 or ay1 < by0 or by1 < ay0, (rects["A"], rects["B"])
    assert near_rect(set_, "full")[1] == tiles_x * tiles_y and near_rect(set_, "empty")[1] == 0


@pytest.mark.parametrize("set_", SET_NAMES)
def test_other_leaves_are_near_and_change_the_isolation_plane(set_):
    for name in ("A", "B"):
        cur, oth, _ = R.split(HC.scene(set_, name)[0], 1)
        assert oth.any()
        d = O.distance_transform(1 - oth, 5)   # distance to the nearest pixel of another leaf
        assert d[cur > 0].min() < 20.0, name
    assert not R.split(HC.scene(set_, "C")[0], 1)[1].any()
    lab = HC.scene(set_, "A")[0]
    ref = O.RefGraspPointSelector()
    default = ref._calculate_isolation_score((lab == 1).astype(np.uint8))
    assert not np.allclose(R.isolation_plane(lab, 1), default, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("set_", SET_NAMES)
def test_the_speckled_frame_overflows_the_small_run_scratch(set_):
    assert HC.runs_of(HC.scene(set_, "over")[0] == 1) > 2 * HC.ORIENT_CAP
    assert HC.runs_of(HC.scene(set_, "A")[0] == 1) < HC.ORIENT_CAP   # (sequence 7 follows the speckled frame with A: no redo)


def test_scenes_are_read_only_and_distinct():
    for set_ in SET_NAMES:
        seen = set()
        for name in HC.ORDER:
            lab, dep = HC.scene(set_, name)
            assert lab.shape == dep.shape == HC.shape_of(set_) and lab.dtype == np.int16 and dep.dtype == np.float32
            assert not lab.flags.writeable and not dep.flags.writeable
            seen.add((lab.tobytes(), dep.tobytes()))
        assert len(seen) == len(HC.ORDER)


def test_every_scripted_step_is_in_the_vocabulary():
    from tests import test_gpu_call_sequences as T

    for set_ in SET_NAMES:
        vocab = HC.vocabulary(set_)
        assert len(set(vocab)) == len(vocab) and {s[0] for s in vocab} == set(HC.ENTRIES)
        for s in vocab:
            assert s[1] == set_ and all(n in HC.ORDER for n in s[2]), s
    names = {(s[0], tuple(k for k, _ in s[3])) for set_ in SET_NAMES for s in HC.vocabulary(set_)}
    n = 0
    for title, (env, steps) in T.SEQUENCES.items():
        for s in steps:
            assert s[0] in HC.ENTRIES and s[1] in HC.SETS and all(x in HC.ORDER for x in s[2]), (title, s)
            assert any(s[0] == e and set(k for k, _ in s[3]) <= set(ks) or s[0] == e and not s[3] for e, ks in names), (title, s)
            n += 1
    assert n > 60
