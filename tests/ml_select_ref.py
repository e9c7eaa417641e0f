"""Test-side reference of the ML-only grasp selection (lg_select_grasp_ml), composed from the oracle's parts: the sample table
restated in NumPy (np.where order, the step rule, the stride grid, the border rule of grasp_point_selector.py:326-328), the
float64 oracle network on RefGraspPointSelector.patch_features at every scored sample, the first-max pick and the centroid."""
import functools

import numpy as np

from oracle import lg_oracle as O

NTH, GRID = 0, 1


@functools.lru_cache(maxsize=None)
def params():
    return O.cnn_closed_form_params(seed=0)


@functools.lru_cache(maxsize=None)
def scene(seed, H, W):
    return O.synthetic_scene(H, W, seed)


def table(mask, mode, target=100, stride=8, max_samples=65536):
    """(n, xy [n, 2] int32, scored [n] int32, (sum x, sum y, area)); n < 0: a GRID frame with more samples than max_samples"""
    H, W = mask.shape
    ys, xs = np.where(mask != 0)
    sums = (int(xs.astype(np.int64).sum()), int(ys.astype(np.int64).sum()), len(ys))
    if mode == NTH:
        step = max(1, len(ys) // target)
        sx, sy = xs[::step], ys[::step]
    else:
        keep = (xs % stride == 0) & (ys % stride == 0)
        sx, sy = xs[keep], ys[keep]
        if len(sx) > max_samples:
            return -len(sx), None, None, sums
    scored = ~((sy < 16) | (sy >= H - 16) | (sx < 16) | (sx >= W - 16))
    return len(sx), np.stack([sx, sy], 1).astype(np.int32).reshape(-1, 2), scored.astype(np.int32), sums


def ref_selector(P, ref_cls=O.RefGraspPointSelector, **kw):
    ref = ref_cls(cnn=None, **kw)
    ref.set_camera_params(P)
    return ref


def oracle_logits(ref, mask, depth, xy, scored):
    """float64 logits of the oracle network at the scored samples (NaN elsewhere)"""
    import torch

    m8 = np.ascontiguousarray(mask, np.uint8)
    with np.errstate(all="ignore"):
        scores = ref._calculate_all_scores(m8, np.asarray(depth, np.float32))
        idx = np.nonzero(scored)[0]
        out = np.full(len(xy), np.nan)
        if len(idx):
            feats = np.stack([ref.patch_features(m8, depth, scores, (int(xy[i, 0]), int(xy[i, 1]))) for i in idx])
            out[idx] = np.asarray(O.cnn_forward(params(), feats, dtype=torch.float64), np.float64)
    return out


def first_max(logits):
    """index of the first sample whose logit is strictly greater than every earlier one's (NaN never wins), -1: none"""
    best, bi = None, -1
    for i, v in enumerate(logits):
        if v != v:
            continue
        if best is None or v > best:
            best, bi = v, i
    return bi


def margin(logits):
    """best logit minus the runner-up among the non-NaN ones (inf with fewer than two)"""
    v = np.sort(np.asarray(logits, np.float64)[~np.isnan(logits)])
    return float(v[-1] - v[-2]) if len(v) >= 2 else float("inf")


def centroid(sums):
    sx, sy, n = sums
    return (sx // n, sy // n)


@functools.lru_cache(maxsize=None)
def case(seed, H, W, leaf, mode, target=100, stride=8):
    """The oracle's view of one leaf of one synthetic scene: mask, depth, P, the table, float64 logits, the pick."""
    labels, depth, P = scene(seed, H, W)
    mask = labels == leaf
    n, xy, scored, sums = table(mask, mode, target, stride)
    ref = ref_selector(P)
    logits = oracle_logits(ref, mask, depth, xy, scored)
    return dict(labels=labels, mask=mask, depth=depth, P=P, n=n, xy=xy, scored=scored, sums=sums, logits=logits, pick=first_max(logits),
                margin=margin(logits), ref=ref)
