"""Shared by tests/test_oracle_params.py and tests/test_gpu_params.py: the scenes of tests/param_sets.py and the oracle run
under a parameter set (CPU only; no device, no product code)."""
import functools

import numpy as np

from oracle import lg_oracle as O
from tests import param_sets as PS


@functools.lru_cache(maxsize=None)
def scene(name):
    """(mask uint8, depth float32, P) of a named scene, or of an (H, W, seed, leaf) tuple."""
    H, W, seed, leaf, *cx = PS.SCENES[name] if isinstance(name, str) else name
    labels, depth, P = O.synthetic_scene(H, W, seed)
    if leaf == "largest":
        ids, counts = np.unique(labels[labels > 0], return_counts=True)
        leaf = int(ids[np.argmax(counts)])
    if leaf == "strip":
        mask = np.zeros((H, W), np.uint8)
        mask[0:36, 100:300] = 1
    else:
        mask = (labels == leaf).astype(np.uint8)
    if cx:
        P = P.copy()
        P[0, 2] = cx[0] * W
    return mask, depth, P


@functools.lru_cache(maxsize=None)
def cnn_params():
    return O.cnn_closed_form_params(seed=0)


def oracle(P, params, with_cnn=False):
    ref = O.RefGraspPointSelector(cnn=(lambda x: O.cnn_forward(cnn_params(), x)) if with_cnn else None, params=params)
    ref.set_camera_params(P)
    return ref


def run(params, scene_name, with_cnn=False):
    """select_grasp_point(return_debug=True) of the oracle under `params` (a full dict) plus every candidate's pre-grasp point."""
    mask, depth, P = scene(scene_name)
    ref = oracle(P, params, with_cnn)
    with np.errstate(all="ignore"):
        triple, dbg = ref.select_grasp_point(mask, depth, return_debug=True)
        if not dbg:   # no candidate at all: the planes are still wanted
            sc = ref._calculate_all_scores(mask, depth)
            dbg = dict(scores=sc, valid=ref._get_valid_regions(mask, sc), candidates=[], ml_scores=[])
        pre = [ref.calculate_pre_grasp_point(ref.get_3d_grasp_point(c, depth), mask) for c in dbg["candidates"]]
    return dict(triple=triple, scores=dbg["scores"], valid=dbg["valid"], candidates=dbg["candidates"],
                ml_scores=dbg["ml_scores"], pregrasp=pre, ref=ref)


@functools.lru_cache(maxsize=None)
def run_set(name, with_cnn=False):
    ps = PS.BY_NAME[name]
    return run(PS.params_of(ps), ps.scene, with_cnn)


@functools.lru_cache(maxsize=None)
def run_baseline(name):
    """What a set must differ from: the defaults (or its `versus`) on the same scene and mask type."""
    ps = PS.BY_NAME[name]
    base = PS.params_of(ps.versus or {})
    base["mask_is_bool"] = PS.params_of(ps)["mask_is_bool"]
    return run(base, ps.scene)


def moved(output, a, b):
    """How far output `output` of run a lies from run b, as (figure, required): a float plane by max |a - b| against 1e-2 of
    its largest magnitude (100 x rtol 1e-4); stem / valid by differing pixels against 50; candidates and the pre-grasp points by
    inequality (1 against 1)."""
    if output in ("stem_penalty", "valid"):
        x, y = (a["valid"], b["valid"]) if output == "valid" else (a["scores"][output], b["scores"][output])
        return int(np.count_nonzero(x != y)), 50
    if output == "candidates":
        return int(a["candidates"] != b["candidates"]), 1
    if output == "pregrasp":
        return int(a["candidates"] == b["candidates"] and a["pregrasp"] != b["pregrasp"]), 1
    x, y = a["scores"][output].astype(np.float64), b["scores"][output].astype(np.float64)
    return float(np.max(np.abs(x - y))), 1e-2 * float(max(np.max(np.abs(x)), np.max(np.abs(y))))


def pick_scores(r):
    """The scores that decide select_grasp_point's pick (:205-236): every candidate's traditional score and, where the CNN
    scored it, its combined score."""
    out = []
    ml = r["ml_scores"] or [None] * len(r["candidates"])
    for (x, y), m in zip(r["candidates"], ml):
        t = float(r["scores"]["traditional_score"][y, x])
        out.append(t)
        if m is not None:
            w = min(0.3, (1.0 - abs(m - 0.5) * 2) * 0.6)
            out.append((1.0 - w) * t + w * m)
    return out


def smallest_relative_gap(values):
    """min over pairs of |a - b| / max(|a|, |b|) (inf for fewer than two values; exact ties give 0)."""
    v = np.sort(np.asarray(values, np.float64))
    if v.size < 2:
        return np.inf
    den = np.maximum(np.abs(v[1:]), np.abs(v[:-1]))
    gap = np.abs(np.diff(v))
    return float(np.min(np.where(den > 0, gap / np.where(den > 0, den, 1), 0.0)))


def walk_gaps(r, top_k, min_distance):
    """The greedy walk of _get_candidate_points (:447-482) over valid_scores = traditional_score * valid, pick by pick: the
    relative gap between the picked pixel and the best OTHER pixel the walk could still have taken at that pick (one that lies
    more than 2 * min_distance from every earlier pick in x or in y -- its neighbours included).  That runner-up is what a
    plane error could put in the picked pixel's place.  Returns [(gap, exact)] per pick: exact = the two scores are the same
    float, a tie that the total order (flat index desc) breaks identically wherever the planes are exact."""
    vs = (r["scores"]["traditional_score"] * r["valid"]).astype(np.float64) + 0.0
    H, W = vs.shape
    free = np.ones((H, W), bool)
    out = []
    cands = r["candidates"]
    assert len(cands) <= top_k
    for (x, y) in cands:
        assert free[y, x]
        s1 = vs[y, x]
        free[y, x] = False
        rest = vs[free]
        if rest.size:
            s2 = float(rest.max())
            assert s2 <= s1
            den = max(abs(s1), abs(s2))
            out.append(((s1 - s2) / den if den > 0 else 0.0, s1 == s2))
        d = 2 * min_distance
        free[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1] = False
    return out
