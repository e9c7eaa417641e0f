"""Ranked grasp candidates without a device: the library's host ranking (lg_rank_grasp_candidates, the code the device kernel runs)
against a Python restatement of the reference's selection loop applied again to what is left, and the row layout of
lg_grasp_candidate against the header."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import leafgrasp_amd as L  # noqa: E402
from leafgrasp_amd import _lib  # noqa: E402


def ref_rank(trad, comb, scored, rescoring):
    """grasp_point_selector.py:205-236 applied successively: each pass starts from the first remaining candidate's traditional
    score and takes every scored remaining candidate whose combined score beats the best so far (Python float comparisons)."""
    remaining = list(range(len(trad)))
    order, picks, by = [], [], []
    while remaining:
        best = remaining[0]
        bs = float(trad[best])
        ml = 0
        if rescoring and len(remaining) > 1:
            for i in remaining:
                if scored[i] and float(comb[i]) > bs:
                    bs, best, ml = float(comb[i]), i, 1
        order.append(best)
        picks.append(bs)
        by.append(ml)
        remaining.remove(best)
    return order, picks, by


def lib_rank(trad, comb, scored, rescoring):
    n = len(trad)
    t = np.ascontiguousarray(trad, np.float64)
    c = np.ascontiguousarray(comb, np.float64)
    s = np.ascontiguousarray(scored, np.int32)
    order, pick, by = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7.0), np.full(max(n, 1), -7, np.int32)
    rc = _lib.lib.lg_rank_grasp_candidates(t.ctypes.data, c.ctypes.data, s.ctypes.data, n, int(rescoring), order.ctypes.data,
                                           pick.ctypes.data, by.ctypes.data)
    assert rc == 0
    return order[:n].tolist(), pick[:n].tolist(), by[:n].tolist()


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _frame(rng, n):
    """Scores on a coarse grid (ties between traditional and combined scores, and among combined scores), NaN traditional
    and combined scores, unscored rows (border candidates of a bool mask)."""
    grid = rng.integers(0, 12, n) / 11.0
    trad = np.where(rng.random(n) < 0.5, grid, rng.random(n))
    comb = np.where(rng.random(n) < 0.5, rng.integers(0, 12, n) / 11.0, rng.random(n))
    if rng.random() < 0.3:
        comb = np.where(rng.random(n) < 0.3, trad, comb)     # a combined score equal to its own traditional score
    trad[rng.random(n) < 0.08] = np.nan
    comb[rng.random(n) < 0.08] = np.nan
    scored = (rng.random(n) < (0.85 if rng.random() < 0.7 else 0.2)).astype(np.int32)
    comb = np.where(scored == 1, comb, np.nan)                 # what the device reports for unscored rows
    return trad, comb, scored


def test_rank_equals_successive_reference_selection():
    rng = np.random.default_rng(11)
    sizes = [0, 1, 64, 2, 3, 20, 63]
    n_frames = 0
    for trial in range(2400):
        n = sizes[trial] if trial < len(sizes) else int(rng.choice([0, 1, 2, 5, 20, 64, int(rng.integers(0, 65))]))
        trad, comb, scored = _frame(rng, n)
        rescoring = bool(rng.random() < 0.8) and n > 1
        exp = ref_rank(trad, comb, scored, rescoring)
        got = lib_rank(trad, comb, scored, rescoring)
        assert got[0] == exp[0], (trial, n, got[0], exp[0])
        assert all(_same(a, b) for a, b in zip(got[1], exp[1])), (trial, got[1], exp[1])
        assert got[2] == exp[2], (trial, got[2], exp[2])
        assert sorted(got[0]) == list(range(n))
        n_frames += 1
    assert n_frames >= 2000


def test_rank_hand_worked():
    # rank 0: 0.6 beats trad[0] = 0.5, 0.95 beats 0.6; rank 1 over {0, 1}: comb[0] = 0.6 beats trad[0]; rank 2: the last one
    # is taken on its traditional score (len(candidates) == 1: no rescoring)
    assert lib_rank([0.5, 0.2, 0.9], [0.6, 0.1, 0.95], [1, 1, 1], True) == ([2, 0, 1], [0.95, 0.6, 0.2], [1, 1, 0])
    # without the CNN the order is the candidate order and every pick is its traditional score
    assert lib_rank([0.5, 0.2, 0.9], [0.6, 0.1, 0.95], [1, 1, 1], False) == ([0, 1, 2], [0.5, 0.2, 0.9], [0, 0, 0])
    # a tie does not replace (strictly greater), the first of equal combined scores wins
    assert lib_rank([0.5, 0.5, 0.5], [0.5, 0.7, 0.7], [1, 1, 1], True)[0] == [1, 2, 0]
    # a NaN start is never beaten; a NaN combined score never wins
    o, p, b = lib_rank([float("nan"), 0.1, 0.2], [0.9, 0.9, float("nan")], [1, 1, 1], True)
    assert o[0] == 0 and math.isnan(p[0]) and b[0] == 0
    assert o[1:] == [1, 2] and p[1:] == [0.9, 0.2] and b[1:] == [1, 0]
    # unscored rows are read for their traditional score only
    assert lib_rank([0.1, 0.2], [0.9, 0.95], [1, 0], True) == ([0, 1], [0.9, 0.2], [1, 0])


def test_rank_rejects_bad_sizes():
    z = np.zeros(65)
    i = np.zeros(65, np.int32)
    for n in (-1, 65):
        assert _lib.lib.lg_rank_grasp_candidates(z.ctypes.data, z.ctypes.data, i.ctypes.data, n, 1, i.ctypes.data, z.ctypes.data,
                                                 i.ctypes.data) == _lib.LG_ERR_INVALID
    assert _lib.lib.lg_rank_grasp_candidates(None, None, None, 0, 1, None, None, None) == 0
    assert _lib.lib.lg_rank_grasp_candidates(None, None, None, 3, 1, None, None, None) == _lib.LG_ERR_INVALID


def test_candidate_struct_matches_header_layout():
    assert C.sizeof(_lib.LgGraspCandidate) == 68 == 17 * 4
    hdr = open(os.path.join(REPO, "include", "leafgrasp.h")).read()
    body = re.search(r"typedef struct lg_grasp_candidate \{(.*?)\} lg_grasp_candidate;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in fields] == [n for n, _ in _lib.LgGraspCandidate._fields_]
    for (name, ctype), (pname, ptype) in zip(fields, _lib.LgGraspCandidate._fields_):
        assert (ctype == "float") == (ptype is C.c_float), name
    dt = L.GRASP_CANDIDATE_DTYPE
    assert dt.itemsize == 68 and list(dt.names) == [n for n, _ in fields]
    for k, (name, ctype) in enumerate(fields):
        assert dt.fields[name][1] == 4 * k == getattr(_lib.LgGraspCandidate, name).offset
        assert dt.fields[name][0] == (np.float32 if ctype == "float" else np.int32)
    # the result row is unchanged
    assert C.sizeof(_lib.LgGraspResult) == 56


def test_selector_exposes_the_candidate_calls():
    for name in ("select_grasp_candidates", "select_grasp_candidates_batch", "select_grasp_candidates_for_leaves"):
        assert callable(getattr(L.GraspPointSelector, name))
    for name in ("lg_select_grasp_candidates", "lg_select_grasp_candidates_labels", "lg_rank_grasp_candidates"):
        assert name in _lib.SYMBOLS


def lib_combine(logit, trad):
    ml, conf, comb = C.c_double(-7.0), C.c_double(-7.0), C.c_double(-7.0)
    assert _lib.lib.lg_ml_combined_score(float(logit), float(trad), C.byref(ml), C.byref(conf), C.byref(comb)) == 0
    return ml.value, conf.value, comb.value


def ref_combine(logit, trad):
    """grasp_point_selector.py:133-136 and :222-226 as the reference writes them: the sigmoid as torch computes it (0 at -inf,
    where math.exp would raise), then Python floats and Python's min."""
    with np.errstate(over="ignore"):
        s = float(1.0 / (1.0 + np.exp(-np.float64(logit))))
    ml = float(np.tanh(s * 3.0) * 0.5 + 0.5)
    conf = 1.0 - abs(ml - 0.5) * 2
    w = min(0.3, conf * 0.6)
    return ml, conf, (1.0 - w) * trad + w * ml


@pytest.mark.parametrize("trad", [0.0, 0.37, 0.9, 1.5])
def test_combined_score_of_a_non_finite_logit(trad):
    """A NaN logit (a non-finite value in the candidate's window) gives NaN ml, confidence and combined score: Python's
    min(0.3, nan) is 0.3 and so is fmin's, and 0.3 * nan is NaN.  +Inf gives ml = tanh(3)/2 + 1/2, -Inf gives 0.5."""
    assert min(0.3, float("nan")) == 0.3
    for nan in (float("nan"), -float("nan")):
        got = lib_combine(nan, trad)
        assert all(math.isnan(v) for v in got), got
        assert all(math.isnan(v) for v in ref_combine(nan, trad))
    for logit, ml in ((math.inf, math.tanh(3.0) / 2 + 0.5), (-math.inf, 0.5)):
        got, exp = lib_combine(logit, trad), ref_combine(logit, trad)
        assert exp[0] == pytest.approx(ml, rel=0, abs=1e-15)
        np.testing.assert_allclose(got, exp, rtol=0, atol=1e-15)
    for logit in (-40.0, -1.0, 0.0, 0.3, 25.0):    # finite control: the same expression
        np.testing.assert_allclose(lib_combine(logit, trad), ref_combine(logit, trad), rtol=0, atol=1e-15)
    got = lib_combine(0.3, float("nan"))           # a NaN traditional score: ml and confidence finite, combined NaN
    assert not math.isnan(got[0]) and not math.isnan(got[1]) and math.isnan(got[2])


def test_rank_with_nan_combined_scores_off_rank_0():
    """NaN combined scores (scored candidates whose window held a hole) at candidates other than 0: a NaN never wins, such a
    candidate is only ever taken on its traditional score as the first one left, and the finite ones order as they do when
    the NaN rows are unscored."""
    nan = float("nan")
    trad = [0.50, 0.45, 0.40, 0.35, 0.30, 0.25]
    comb = [0.52, nan, 0.70, nan, 0.60, nan]
    scored = [1] * 6
    exp = ref_rank(trad, comb, scored, True)
    got = lib_rank(trad, comb, scored, True)
    assert got == exp
    assert got[0] == [2, 4, 0, 1, 3, 5] and got[1] == [0.70, 0.60, 0.52, 0.45, 0.35, 0.25] and got[2] == [1, 1, 1, 0, 0, 0]
    for r, i in enumerate(got[0]):
        if math.isnan(comb[i]):
            assert got[2][r] == 0 and got[1][r] == trad[i]
    # the same list with the NaN rows unscored instead: the same order and picks
    unscored = [0 if math.isnan(c) else 1 for c in comb]
    assert lib_rank(trad, comb, unscored, True) == got
    # randomised: NaN combined scores anywhere but at candidate 0, finite traditional scores
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(2, 65))
        t = rng.random(n)
        c = rng.random(n)
        holes = rng.random(n) < 0.4
        holes[0] = False
        c[holes] = np.nan
        s = np.ones(n, np.int32)
        o, p, b = lib_rank(t, c, s, True)
        assert (o, p, b) == ref_rank(t, c, s, True), trial
        assert not any(math.isnan(v) for v in p)
        assert all(b[r] == 0 and p[r] == t[i] for r, i in enumerate(o) if holes[i]), trial
        assert (o, p, b) == lib_rank(t, c, (~holes).astype(np.int32), True), trial


@pytest.mark.parametrize("n", [1, 2, 64])
def test_rank_all_ties(n):
    order, pick, by = lib_rank([0.25] * n, [0.25] * n, [1] * n, n > 1)
    assert order == list(range(n)) and pick == [0.25] * n and by == [0] * n
