"""CPU side of tests/test_gpu_train_hparams.py: the table of whole-step cases off the default hyper-parameters, their
seeded inputs, and the precondition on their seeds.

A training step is not continuous in its inputs (ReLU / max-pool decisions, tests/test_train_oracle.py), so the oracle in
float32 and the oracle in float64 can themselves disagree on a case.  A seed is only used where they agree within HALF of
compare_step's tight bounds: then a device result outside those bounds cannot be blamed on the reference's conditioning."""
import numpy as np
import pytest

import synthetic_inputs as S
from oracle import lg_oracle as O

torch = pytest.importorskip("torch")

DEFAULTS = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0, pos_weight=2.0)
HP_SETS = {
    "noclip_pw7.5": dict(max_grad_norm=0.0, pos_weight=7.5),
    "nodecay_pw0.5": dict(weight_decay=0.0, pos_weight=0.5),
    "all_off": dict(lr=1e-3, betas=(0.8, 0.9), eps=1e-3, weight_decay=0.1, max_grad_norm=0.5, pos_weight=1.0),
    "defaults": {},
}
SMALL, STANDARD = (32, 64, 128), (64, 128, 256)
# (hyper-parameter set, encoder, N, seed).  The seed is the first of 0..9 that passes test_step_case_seed_is_well_conditioned
# with margin, at 1, 2 and 8 threads of the float32 oracle (profiles/NOTES_train_tests.md lists every seed's figures).
# There is no N = 2 case: at N = 2 the float32 oracle's agreement with the float64 one depends on the host and its thread
# count (seed 0: 0.27 on one host, 1.09 on another, 5.49 with one thread; no seed of 0..9 qualifies everywhere), so a
# comparison with it could blame the kernel for the reference.  N = 3 is the smallest batch held to the oracle; N = 2 is
# held bit for bit by the mask, sequence and loss tests.
STEP_CASES = [
    ("noclip_pw7.5", SMALL, 16, 0), ("noclip_pw7.5", STANDARD, 16, 0),
    ("nodecay_pw0.5", SMALL, 16, 0), ("nodecay_pw0.5", STANDARD, 16, 0),
    ("all_off", SMALL, 16, 0), ("all_off", STANDARD, 16, 0),
    ("defaults", SMALL, 3, 0), ("defaults", STANDARD, 3, 0),
]


def case_id(case):
    hp, filt, n, seed = case
    return f"{hp}-{filt[0]}-n{n}-s{seed}"


def hparams(name):
    return {**DEFAULTS, **HP_SETS[name]}


def step_case_inputs(filt, n, seed, att="spatial"):
    """params, x, y, masks of a seeded case (the recipe of test_train_step_with_dropout_masks_vs_oracle)."""
    from tests.test_gpu_train import random_masks
    params = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    x = S.synthetic_patches(n, seed=20 + seed)
    y = (np.random.default_rng(seed).random(n) < 0.4).astype(np.float32)
    y[0], y[1] = 0.0, 1.0
    return params, x, y, random_masks(filt, n, seed)


def conditioning(r32, r64):
    """Disagreement of two oracle results as a fraction of compare_step's tight bounds (1.0 = at the bound), criterion
    by criterion; the gradient rules are compare_step's own, tensor by tensor."""
    out = {"loss": abs(r32["loss"] - r64["loss"]) / (2e-5 * abs(r64["loss"])),
           "logits": float(np.max(np.abs(r32["logits"] - r64["logits"]) / (2e-5 + 1e-4 * np.abs(r64["logits"])))),
           "grad_norm": abs(r32["grad_norm"] - r64["grad_norm"]) / (2e-4 * abs(r64["grad_norm"]))}
    worst, worst_cls, worst_zero = 0.0, 0.0, 0.0
    for k, gr in r64["grads"].items():
        den = float(np.linalg.norm(gr))
        g = r32["grads"][k].astype(np.float64)
        if den < 1e-4 * r64["grad_norm"] / np.sqrt(len(r64["grads"])):
            worst_zero = max(worst_zero, float(np.abs(g).max()) / (1e-4 * max(1.0, r64["grad_norm"])))
            continue
        e = float(np.linalg.norm(g - gr)) / den
        worst = max(worst, e / 2e-2)
        if k.startswith("classifier"):
            worst_cls = max(worst_cls, e / 2e-4)
    out.update(grads=worst, classifier_grads=worst_cls, zero_grads=worst_zero)
    return out


def oracle_pair(hp_name, filt, n, seed):
    params, x, y, masks = step_case_inputs(filt, n, seed)
    hp = hparams(hp_name)
    return (O.cnn_train_step(params, x, y, masks=masks, **hp),
            O.cnn_train_step(params, x, y, masks=masks, dtype=torch.float64, **hp))


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_step_case_seed_is_well_conditioned(case):
    hp_name, filt, n, seed = case
    c = conditioning(*oracle_pair(hp_name, filt, n, seed))
    print(case_id(case), {k: round(v, 4) for k, v in c.items()})
    assert max(c.values()) <= 0.5, c


def test_hp_sets_leave_the_defaults():
    """(i) and (ii) are the sets the issue names; every set differs from the defaults in what it says it does."""
    assert hparams("noclip_pw7.5")["max_grad_norm"] == 0.0 and hparams("noclip_pw7.5")["pos_weight"] == 7.5
    assert hparams("nodecay_pw0.5")["weight_decay"] == 0.0 and hparams("nodecay_pw0.5")["pos_weight"] == 0.5
    assert all(hparams("all_off")[k] != v for k, v in DEFAULTS.items())
    assert hparams("defaults") == DEFAULTS
