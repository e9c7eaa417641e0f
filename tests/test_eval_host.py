"""CPU tests (no GPU) of the validation metrics' host twin, lg_eval_logits_host -- the code the device kernels run -- and of
trainer.metrics_from_counts, against the reference-generated pair of tests/golden/train_host_vectors.npz (ap_outputs,
ap_labels, ap_metrics: analyze_predictions of scripts/train_model.py:64-99) and against torch's float64
binary_cross_entropy_with_logits taken per chunk and averaged (train_model.py:280-306).

Loss tolerance 1e-12 * max(1, |ref|), derived: every term is a non-negative loss term; its error is a few double ulps plus
ulp(|z|) from the z - z cancellation at large |z|; with |z| <= 30 the averaged error stays below 1e-14, so 1e-12 leaves a
factor of 100, while a wrong formula or a wrong chunking is off by 1e-3 or more."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from leafgrasp_amd import _lib
from leafgrasp_amd.trainer import analyze_predictions, metrics_from_counts

HERE = os.path.dirname(os.path.abspath(__file__))
_FP = C.POINTER(C.c_float)
KEYS = ("positive_accuracy", "negative_accuracy", "precision", "recall", "f1_score")


def host_eval(z, y, chunk=16, pw=2.0, thr=0.5):
    z, y = np.ascontiguousarray(z, np.float32).reshape(-1), np.ascontiguousarray(y, np.float32).reshape(-1)
    r = _lib.LgEvalResult()
    rc = _lib.lib.lg_eval_logits_host(z.ctypes.data_as(_FP), y.ctypes.data_as(_FP), z.size, chunk, pw, thr, C.byref(r))
    assert rc == 0, rc
    return r


def torch_loss(z, y, chunk, pw):
    """float64 BCEWithLogitsLoss(pos_weight) per chunk, the chunk means averaged (train_model.py:285, :306)."""
    zt, yt = torch.from_numpy(np.asarray(z, np.float64).reshape(-1)), torch.from_numpy(np.asarray(y, np.float64).reshape(-1))
    w = torch.tensor([pw], dtype=torch.float64)
    means = [torch.nn.functional.binary_cross_entropy_with_logits(zt[s:s + chunk], yt[s:s + chunk], pos_weight=w).item()
             for s in range(0, zt.shape[0], chunk)]
    return float(np.mean(means)), len(means)


def counts_ref(z, y, thr):
    z, y = np.asarray(z, np.float32).reshape(-1), np.asarray(y, np.float32).reshape(-1)
    pred = z > np.float32(thr)
    tp, tn = int((pred & (y == 1)).sum()), int((~pred & (y == 0)).sum())
    return tp, int((y == 0).sum()) - tn, int((y == 1).sum()) - tp, tn, int(((z > 0) == (y == 1)).sum())


@pytest.fixture(scope="module")
def pair():
    g = np.load(os.path.join(HERE, "golden", "train_host_vectors.npz"))
    return g["ap_outputs"], g["ap_labels"], g["ap_metrics"]


def test_struct_is_64_bytes():
    assert C.sizeof(_lib.LgEvalResult) == 64


def test_golden_pair(pair):
    z, y, m = pair
    r = host_eval(z, y, 16, 2.0, 0.5)
    assert (r.tp, r.fp, r.fn, r.tn) == (6, 7, 16, 11) == tuple(int(v) for v in m[5:9])
    assert (r.n, r.n_chunks) == (40, 3)   # chunks of 16, 16 and 8
    got = metrics_from_counts(r.tp, r.fp, r.fn, r.tn)
    for k, v in zip(KEYS, m[0:5]):
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
    assert got == analyze_predictions(torch.from_numpy(z), torch.from_numpy(y))   # same keys, same values
    ref, nch = torch_loss(z, y, 16, 2.0)
    assert nch == 3
    print("loss", repr(r.loss), "torch float64", repr(ref))
    assert abs(r.loss - ref) <= 1e-12 * max(1.0, abs(ref))
    assert r.correct == counts_ref(z, y, 0.5)[4]
    # the short last chunk weighs as much as a full one: the mean over all 40 samples is another number
    assert abs(torch_loss(z, y, 40, 2.0)[0] - ref) > 1e-3


@pytest.mark.parametrize("n,chunk", [(1, 16), (16, 16), (5, 16), (37, 16), (37, 1), (37, 37)])
def test_shapes(n, chunk):
    rng = np.random.default_rng(100 + n)
    z = (rng.standard_normal(n) * 4).astype(np.float32)
    y = (rng.random(n) < 0.4).astype(np.float32)
    for pw, thr in ((2.0, 0.5), (1.0, 0.0), (3.5, -0.25)):
        r = host_eval(z, y, chunk, pw, thr)
        ref, nch = torch_loss(z, y, chunk, pw)
        assert (r.n, r.n_chunks) == (n, nch) and nch == -(-n // chunk)
        assert abs(r.loss - ref) <= 1e-12 * max(1.0, abs(ref)), (r.loss, ref)
        assert (r.tp, r.fp, r.fn, r.tn, r.correct) == counts_ref(z, y, thr)
        assert r.tp + r.fp + r.fn + r.tn == n


def test_large_logits_do_not_overflow():
    z = np.array([30.0, -30.0, 30.0, -30.0, 0.0], np.float32)
    y = np.array([1, 0, 0, 1, 1], np.float32)
    r = host_eval(z, y, 16, 2.0, 0.5)
    ref, _ = torch_loss(z, y, 16, 2.0)
    assert math.isfinite(r.loss) and abs(r.loss - ref) <= 1e-12 * max(1.0, abs(ref))


@pytest.mark.parametrize("label", [1.0, 0.0])
def test_one_class_only(label):
    """All-positive / all-negative labels: the zero denominators of analyze_predictions give 0, not an error."""
    rng = np.random.default_rng(7)
    z = rng.standard_normal(21).astype(np.float32)
    y = np.full(21, label, np.float32)
    r = host_eval(z, y)
    assert (r.tp, r.fp, r.fn, r.tn, r.correct) == counts_ref(z, y, 0.5)
    assert (r.fp + r.tn == 0) if label == 1.0 else (r.tp + r.fn == 0)
    got = metrics_from_counts(r.tp, r.fp, r.fn, r.tn)
    assert got == analyze_predictions(torch.from_numpy(z), torch.from_numpy(y))
    assert got["negative_accuracy" if label == 1.0 else "positive_accuracy"] == 0
    assert metrics_from_counts(0, 0, 5, 0)["f1_score"] == 0 and metrics_from_counts(0, 0, 0, 0)["precision"] == 0


def test_nan_logit_follows_ieee():
    z = np.array([1.0, np.nan, -2.0, 0.7], np.float32)
    y = np.array([1, 1, 0, 0], np.float32)
    r = host_eval(z, y, 2)
    assert math.isnan(r.loss)
    assert (r.tp, r.fp, r.fn, r.tn) == (1, 1, 1, 1)      # the NaN is not predicted positive: a false negative
    assert r.correct == 2                                # 1.0 / label 1 and -2.0 / label 0; NaN > 0 is false, label 1
    # a NaN in one chunk poisons the mean of the chunk means
    assert math.isnan(host_eval(z, y, 1).loss)


def test_bad_arguments():
    z = np.zeros(4, np.float32)
    p, r = z.ctypes.data_as(_FP), _lib.LgEvalResult()
    f = _lib.lib.lg_eval_logits_host
    assert f(p, p, 0, 16, 2.0, 0.5, C.byref(r)) == _lib.LG_ERR_INVALID
    assert f(p, p, -3, 16, 2.0, 0.5, C.byref(r)) == _lib.LG_ERR_INVALID
    assert f(p, p, 4, 0, 2.0, 0.5, C.byref(r)) == _lib.LG_ERR_INVALID
    assert f(None, p, 4, 16, 2.0, 0.5, C.byref(r)) == _lib.LG_ERR_INVALID
    assert f(p, None, 4, 16, 2.0, 0.5, C.byref(r)) == _lib.LG_ERR_INVALID
    assert f(p, p, 4, 16, 2.0, 0.5, None) == _lib.LG_ERR_INVALID
