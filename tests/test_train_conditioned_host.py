"""The premises of tests/test_gpu_train_conditioned.py, on the CPU (profiles/NOTES_train_conditioned.md).

The conditioned cases of tests/golden/train_conditioned.npz are first training steps whose every ReLU / max-pool site is at
least tau away from its tie, so that a float32 implementation takes the float64 decisions and can be held to the float64
oracle at rounding.  Here: the helper that exposes the decisions is the oracle's network; the margins are there (recomputed);
the nudges are small; torch's float32 does take the float64 decisions and deviates locally by at most tau / 32; the new
bounds see two defects the 2 % bound does not; and one flipped decision breaks them (why conditioning is needed)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import lg_oracle as O
from tests import train_decisions_ref as D

IDS = [D.case_tag(*c) for c in D.CASES]


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(D.FIXTURE)


@functools.lru_cache(maxsize=None)
def conditioned(case):
    """(inputs, float64 helper result, float64 oracle result, bounds) of a conditioned case; computed once, never modified."""
    fx = fixture()
    inputs = D.conditioned_inputs(fx, *case)
    params, x, y, mk = inputs
    ref = D.oracle_step(O, params, x, y, mk, torch.float64)
    return inputs, D.step(params, x, y, mk), ref, D.bounds(fx, D.case_tag(*case), ref)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def test_cases_and_masks_follow_the_trainer():
    from leafgrasp_amd.trainer import dropout_layout
    for att, filt, n in D.CASES:
        mk = D.keep_masks(filt, n, 1)
        assert [m.shape for m in mk] == [(n, w) for w, _ in dropout_layout(filt)]
        for m, (_, p) in zip(mk, dropout_layout(filt)):
            assert set(np.unique(m)) <= {np.float32(0.0), np.float32(1.0 / (1.0 - p))}
    assert len(set(IDS)) == len(D.CASES) and float(fixture()["tau_factor"]) == 64.0


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_helper_is_the_oracles_network(case):
    """decisions=None: logits and gradients of O.cnn_train_step(dtype=float64) to 1e-12 relative, so the margins are those of
    the oracle's network; the override with the decisions it took itself changes nothing."""
    (params, x, y, mk), r, ref, _ = conditioned(case)
    np.testing.assert_allclose(r["logits"], ref["logits"], rtol=1e-12, atol=1e-12 * np.abs(ref["logits"]).max())
    assert r["loss"] == pytest.approx(ref["loss"], rel=1e-12)
    for k, g in ref["grads"].items():
        np.testing.assert_allclose(r["grads"][k], g, rtol=0, atol=1e-12 * max(np.abs(g).max(), 1e-12 * ref["grad_norm"]), err_msg=k)
    for k, v in r["buffers"].items():
        np.testing.assert_allclose(v, ref["params"][k], rtol=1e-12, atol=1e-15, err_msg=k)
    assert list(r["z"]) + list(r["gap"]) and set(r["z"]) | set(r["gap"]) == set(D.site_groups(params))
    forced = D.step(params, x, y, mk, decisions=r["decisions"])
    for k, g in ref["grads"].items():
        np.testing.assert_allclose(forced["grads"][k], g, rtol=0, atol=1e-12 * max(np.abs(g).max(), 1e-12 * ref["grad_norm"]), err_msg=k)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_every_site_is_clear_and_nudges_are_small(case):
    fx, tag = fixture(), D.case_tag(*case)
    (params, *_), r, _, _ = conditioned(case)
    groups = [str(g) for g in fx[f"{tag}_group"]]
    assert groups == D.site_groups(params)
    m = D.margins(r)
    for g, tau in zip(groups, fx[f"{tag}_tau"]):
        assert m[g] >= tau > 0, (g, m[g], tau)
    # a pool cell without a positive entry is no site; every other cell is one
    for g, gap in r["gap"].items():
        zz = D.pool_cells(torch.from_numpy(r["z"]["encoder." + g.split(".")[1] + ".4"])).numpy()
        np.testing.assert_array_equal(np.isinf(gap), zz.max(axis=-1) <= 0)
    delta = fx[f"{tag}_nudge_delta"]
    assert 0 < len(delta) == len(fx[f"{tag}_nudge_name"]) == len(fx[f"{tag}_nudge_index"])
    assert float(np.abs(delta).max()) <= 1e-2
    steps = delta.astype(np.float64) / 1e-3
    np.testing.assert_allclose(steps, np.round(steps), atol=1e-4)      # multiples of 1e-3
    touched = {str(k).rsplit(".", 1)[0].split(".")[0] + "/" + str(k).rsplit(".", 1)[1] for k in fx[f"{tag}_nudge_name"]}
    assert touched <= {"encoder/bias", "encoder/weight", "classifier/bias", "attention/bias", "channel_attention/bias"}
    print(f"{tag}: {len(delta)} nudged parameters, {int(fx[f'{tag}_tries'].sum())} tries")


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_float32_oracle_takes_the_float64_decisions(case):
    fx, tag = fixture(), D.case_tag(*case)
    (params, x, y, mk), r, _, _ = conditioned(case)
    r32 = D.step(params, x, y, mk, dtype=torch.float32, want_grads=False)
    for g, keep in r["decisions"]["relu"].items():
        np.testing.assert_array_equal(r32["decisions"]["relu"][g], keep, err_msg=g)
    for g, arg in r["decisions"]["pool"].items():
        site = np.isfinite(r["gap"][g])
        np.testing.assert_array_equal(r32["decisions"]["pool"][g][site], arg[site], err_msg=g)
    dev = D.local_deviation(r32, r)
    for g, tau in zip(fx[f"{tag}_group"], fx[f"{tag}_tau"]):
        assert tau >= 32.0 * dev[str(g)], (g, tau, dev[str(g)])


def conv_without_pixel00(h, w, b, padding):
    """The conv whose WEIGHT gradient lacks output pixel (0, 0) of every sample; values and input gradient unchanged."""
    keep = torch.ones_like(h[:1, :1])
    keep[..., 0, 0] = 0
    return F.conv2d(h, w, b, padding=padding) * keep + F.conv2d(h, w.detach(), b, padding=padding) * (1 - keep)


class _BatchNormDividingByMMinus1(torch.autograd.Function):
    """Train-mode BatchNorm2d whose backward takes the two batch means of dx over M - 1 for M."""

    @staticmethod
    def forward(ctx, h, gamma, beta):
        mean = h.mean(dim=(0, 2, 3), keepdim=True)
        inv = 1.0 / torch.sqrt(h.var(dim=(0, 2, 3), unbiased=False, keepdim=True) + 1e-5)
        xh = (h - mean) * inv
        ctx.save_for_backward(xh, inv, gamma)
        return xh * gamma[None, :, None, None] + beta[None, :, None, None]

    @staticmethod
    def backward(ctx, dy):
        xh, inv, gamma = ctx.saved_tensors
        m = dy.shape[0] * dy.shape[2] * dy.shape[3]
        dbeta, dgamma = dy.sum(dim=(0, 2, 3)), (dy * xh).sum(dim=(0, 2, 3))
        dx = gamma[None, :, None, None] * inv * (dy - (dbeta / (m - 1))[None, :, None, None] - xh * (dgamma / (m - 1))[None, :, None, None])
        return dx, dgamma, dbeta


def bn_dividing_by_m_minus_1(h, rm, rv, gamma, beta, *_):
    return _BatchNormDividingByMMinus1.apply(h, gamma, beta)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_the_bound_sees_what_two_percent_does_not(case):
    """Two gradients computed on purpose with a defect, by autograd in float64: both stay inside compare_step's 2 % and both
    are more than ten times outside the new bound of their tensor."""
    (params, x, y, mk), r, _, bound = conditioned(case)
    nb = len(case[1])
    defects = (("encoder.0.3.weight", {"conv:encoder.0.3": conv_without_pixel00}),
               ("encoder.1.1.weight", {f"bn:encoder.{b}.{k}": bn_dividing_by_m_minus_1 for b in range(nb) for k in (1, 4)}))
    for k, ops in defects:
        bad = D.step(params, x, y, mk, ops=ops)
        np.testing.assert_allclose(bad["logits"], r["logits"], rtol=1e-12, atol=1e-12)      # the forward is untouched
        e = rel_l2(bad["grads"][k], r["grads"][k])
        print(f"{D.case_tag(*case)}: {k} with the defect {e:.3e}, new bound {bound['grad_l2/' + k]:.3e}")
        assert 10.0 * bound["grad_l2/" + k] < e < 2e-2, (k, e, bound["grad_l2/" + k])


def closest_site(r, taus, mk):
    """(group, flat index or (cell, second arg-max)) of the site with the smallest margin in units of its group's tau, among
    the sites that carry gradient: a (sample, channel) plane that Dropout2d drops behind the pool carries none, nor does an
    entry in front of a pool that is not its cell's maximum."""
    best = None
    for g, z in r["z"].items():
        a = np.abs(z)
        if g.startswith("encoder.") and g.endswith(".4"):      # in front of a pool: only a kept cell maximum carries gradient
            b = g.split(".")[1]
            where = D.pool_cells(torch.arange(z.size).reshape(z.shape)).numpy()
            arg = r["decisions"]["pool"]["pool." + b][..., None]
            live = np.zeros(z.size, bool)
            live[np.take_along_axis(where, arg, -1).reshape(-1)] = True
            a = np.where(live.reshape(z.shape) & (z > 0) & (mk[int(b)][:, :, None, None] > 0), a, np.inf)
        i = int(a.argmin())
        cand = (float(a.reshape(-1)[i]) / taus[g], g, i)
        best = cand if best is None or cand < best else best
    for g, gap in r["gap"].items():
        gap = np.where(mk[int(g.split(".")[1])][:, :, None, None] > 0, gap, np.inf)
        i = int(gap.argmin())
        zz = D.pool_cells(torch.from_numpy(np.maximum(r["z"]["encoder." + g.split(".")[1] + ".4"], 0))).numpy().reshape(-1, 4)[i]
        cand = (float(gap.reshape(-1)[i]) / taus[g], g, (i, int(np.argsort(zz)[-2])))
        best = cand if cand < best else best
    return best


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_one_flipped_decision_breaks_the_bound(case):
    """Why conditioning is needed: the single closest site decided the other way moves some tensor by more than ten times its
    new bound (and, as compare_step's comment says, by less than 2 %)."""
    fx, tag = fixture(), D.case_tag(*case)
    (params, x, y, mk), r, _, bound = conditioned(case)
    taus = dict(zip((str(g) for g in fx[f"{tag}_group"]), fx[f"{tag}_tau"]))
    ratio, group, where = closest_site(r, taus, mk)
    flipped = D.step(params, x, y, mk, decisions=D.flip_site(r["decisions"], group, where))
    worst = max((rel_l2(flipped["grads"][k], g) / bound["grad_l2/" + k], k) for k, g in r["grads"].items()
                if np.linalg.norm(g) > 1e-4 * np.sqrt(sum(float((v ** 2).sum()) for v in r["grads"].values()) / len(r["grads"])))
    print(f"{tag}: closest site {group} at {ratio:.2f} tau; flipped: {worst[1]} at {worst[0]:.1f} x its bound")
    assert worst[0] > 10.0, (group, where, worst)
