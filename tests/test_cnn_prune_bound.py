"""The bound behind lg_select_grasp's CNN pruning, without a device: whenever the library's predicate
(lg_cnn_candidate_cannot_win) says that a candidate with traditional score trad_i cannot beat candidate 0's trad_0, the
library's own rescoring formula (lg_ml_combined_score, the code the device runs) gives combined <= trad_0 for EVERY logit; a
NaN or an infinite score is never pruned; and the predicate does prune just above the analytic bound (it is not quietly loose).
"""
import ctypes as C
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402

ML_MAX = 0.5 + math.tanh(3.0) / 2


def combined(logit, trad):
    ml, conf, comb = C.c_double(), C.c_double(), C.c_double()
    assert _lib.lib.lg_ml_combined_score(float(logit), float(trad), C.byref(ml), C.byref(conf), C.byref(comb)) == 0
    return ml.value, conf.value, comb.value


def cannot_win(ti, t0):
    return bool(_lib.lib.lg_cnn_candidate_cannot_win(float(ti), float(t0)))


def upper_bound(t):
    """max over ml in [0.5, 1] of (1 - w) t + w ml, w = min(0.3, 0.6 (1 - 2 |ml - 0.5|))."""
    return 0.7 * t + 0.225 if t < 0.5 else t + 0.3 * (1.0 - t) ** 2


def maximising_logit(t):
    """The logit whose ml is the maximiser of the combined score: 0.75 below trad 0.5, (1 + trad) / 2 above (clipped to what
    tanh(3 sigmoid) reaches)."""
    ml = 0.75 if t < 0.5 else min((1.0 + t) / 2.0, ML_MAX)
    sg = math.atanh(min(2.0 * ml - 1.0, 1.0 - 1e-16)) / 3.0
    if sg >= 1.0:
        return 60.0
    return math.log(sg / (1.0 - sg))


def _trads():
    rng = np.random.default_rng(7)
    grid = np.linspace(-1.0, 2.0, 301)
    rnd = rng.uniform(-1.0, 2.0, 150).astype(np.float32).astype(np.float64)
    near = rng.uniform(0.7, 0.95, 50).astype(np.float32).astype(np.float64)   # where the benchmark's candidates lie
    return np.concatenate([grid, rnd, near])


LOGITS = np.concatenate([np.linspace(-60.0, 60.0, 1201), [np.inf, -np.inf, 1e30, -1e30, np.nan]])


def test_formula_is_the_reference_rescoring():
    for logit, trad in ((0.3, 0.8), (-4.0, 0.2), (7.5, 1.3), (0.0, -0.5)):
        ml, conf, comb = combined(logit, trad)
        s = 1.0 / (1.0 + math.exp(-logit))
        m = math.tanh(s * 3.0) * 0.5 + 0.5
        cf = 1.0 - abs(m - 0.5) * 2
        w = min(0.3, cf * 0.6)
        assert ml == m and conf == cf and comb == (1.0 - w) * trad + w * m
    ml, _, comb = combined(float("nan"), 0.5)
    assert math.isnan(ml) and math.isnan(comb) and not comb > 0.0   # a NaN logit is never taken


def test_pruned_candidates_cannot_win_for_any_logit():
    trads = _trads()
    pruned = kept = 0
    worst_slack = np.inf
    for ti in trads:
        combs = np.array([combined(lg, ti)[2] for lg in np.append(LOGITS, maximising_logit(ti))])
        assert np.isnan(combs[-2]) and not np.isnan(np.delete(combs, -2)).any()
        cmax = float(np.nanmax(combs))
        ub = upper_bound(ti)
        assert cmax <= ub + 1e-15 * (1 + abs(ti)), (ti, cmax, ub)     # the analytic bound holds on the library's arithmetic
        if -1.0 <= ti < 0.995:
            assert cmax >= ub - 1.5e-6, (ti, cmax, ub)                # and the logit grid reaches it
        t0s = np.concatenate([trads, [cmax, np.nextafter(cmax, 2), np.nextafter(cmax, -2), ub, ub + 1e-9, ub - 1e-9, ub + 1e-6]])
        for t0 in t0s:
            if cannot_win(ti, t0):
                pruned += 1
                assert cmax <= t0, (ti, t0, cmax)
                worst_slack = min(worst_slack, t0 - cmax)
            else:
                kept += 1
    print(f"{pruned} pruned pairs (smallest trad_0 - max combined: {worst_slack:.3e}), {kept} kept")
    assert pruned > 10000 and kept > 10000


def test_nan_and_infinite_scores_are_never_pruned():
    special = [float("nan"), float("inf"), float("-inf")]
    others = list(_trads()[::25]) + special + [1e300, -1e300]
    for a in special:
        for b in others:
            assert not cannot_win(a, b), (a, b)
            assert not cannot_win(b, a), (b, a)


def test_bound_is_not_loose():
    for ti in _trads():
        ub = upper_bound(ti)
        assert cannot_win(ti, ub + 1e-6), ti
        assert not cannot_win(ti, ub - 1e-6), ti
    assert not cannot_win(0.9, 0.9)          # candidate 0 itself can be lifted above its own traditional score
    assert cannot_win(0.80, 0.90) and not cannot_win(0.899, 0.90)
