"""The training step's gradients held to rounding against the FLOAT64 oracle, on cases conditioned clear of ReLU / max-pool
ties (tests/golden/train_conditioned.npz, tests/train_decisions_ref.py; premises: tests/test_train_conditioned_host.py;
measurements and mutations: profiles/NOTES_train_conditioned.md).

tests/test_gpu_train.py::compare_step allows every gradient tensor 2 % because one decision within rounding of its tie, taken
the other way, moves the tensors below it by ~0.3 %.  On a conditioned case every site is at least tau (64 x torch's local
float32 deviation) from its tie, so the device takes the float64 decisions and the step is smooth: every quantity is held to
4 x the deviation of the float32 oracle from the float64 oracle on the same case (the fixture's yardstick, the largest over
1, 2 and 8 threads), floored at 4 float32 ulps; 8 x for exp_avg_sq and 16 x for the head (loss, gradient norm, the last layer,
one-element biases: sums of the logit errors), see train_decisions_ref.factor and findings 2 and 3 of the notes.  The oracle is
handed the float32 hyper-parameter values the device holds (finding 1).  Everything goes through GraspTrainer and the existing
conv-form switches.

Held per case: per parameter tensor the gradient's relative L2 and largest element-wise deviation (biases in front of a
BatchNorm, whose gradient is mathematically zero: compare_step's rule), logits, loss, gradient norm, every running_mean /
running_var, and exp_avg / exp_avg_sq after the updating step ((1 - beta1) g' and (1 - beta2) g'^2: the gradient and the clip
coefficient once more).  Not held here: the updated parameters (Adam's first update is lr * sign(g); assert_adam_replay holds
the optimiser), second steps, and BatchNorm chunking at 8 x 8 / 4 x 4 (N >= 128: the N = 128 / 258 tests at their bounds)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import train_decisions_ref as D  # noqa: E402
from tests.test_gpu_train import CONV_FORMS, make_trainer  # noqa: E402

FORMS = {"default": {}, **CONV_FORMS}
# N = 13 (ragged against the 4- and 16-sample tiles, BatchNorm chunks of 5 + 5 + 3 samples at 32 x 32) under every conv form;
# N = 3, 16, 33 at the default thresholds
RUNS = [(c, f) for c in D.CASES if c[2] == 13 for f in FORMS] + [(c, "default") for c in D.CASES if c[2] != 13]


@functools.lru_cache(maxsize=None)
def reference(case):
    """Conditioned inputs, the float64 oracle step on them and the bounds; computed once per case, shared, never modified."""
    fx = np.load(D.FIXTURE)
    params, x, y, mk = D.conditioned_inputs(fx, *case)
    ref = D.oracle_step(O, params, x, y, mk, torch.float64)
    return (params, x, y, mk), ref, D.bounds(fx, D.case_tag(*case), ref)


def device_result(tr, loss, logits, gnorm, with_moments):
    sd = tr.state_dict()
    out = {"loss": loss, "grad_norm": gnorm, "logits": logits.cpu().numpy(), "grads": {k: v.numpy() for k, v in tr.gradients().items()},
           "params": {k: v.numpy() for k, v in sd.items() if "running_" in k}, "opt_state": {"exp_avg": {}, "exp_avg_sq": {}}}
    if with_moments:
        opt = tr.optimizer_state()
        out["opt_state"] = {key: {k: v.numpy() for k, v in opt[key].items()} for key in ("exp_avg", "exp_avg_sq")}
    return out


@pytest.mark.parametrize("case,form", RUNS, ids=[f"{D.case_tag(*c)}-{f}" for c, f in RUNS])
def test_conditioned_step_vs_float64_oracle(monkeypatch, case, form):
    att, filt, n = case
    (params, x, y, mk), ref, bound = reference(case)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    tr = make_trainer(att, filt, max(16, n))
    for k in FORMS[form]:
        monkeypatch.delenv(k)
    state = {k: torch.from_numpy(v) for k, v in params.items()}
    tr.load_state_dict(state)
    got = device_result(tr, *tr.train_step(x, y, masks=mk, apply_update=False, return_logits=True), with_moments=False)
    assert tr.optimizer_state()["step"] == 0
    tr.load_state_dict(state)          # the running statistics back to the case's: the updating step is a first step too
    upd = device_result(tr, *tr.train_step(x, y, masks=mk, return_logits=True), with_moments=True)
    assert tr.optimizer_state()["step"] == 1
    # the two steps saw the same inputs: same bits (every reduction of the path is ordered)
    assert (got["loss"], got["grad_norm"]) == (upd["loss"], upd["grad_norm"])
    np.testing.assert_array_equal(got["logits"], upd["logits"])
    for k in got["grads"]:
        np.testing.assert_array_equal(got["grads"][k], upd["grads"][k], err_msg=k)
    for k in got["params"]:
        np.testing.assert_array_equal(got["params"][k], upd["params"][k], err_msg=k)
    dev = D.yardstick_quantities(upd, ref)
    assert set(dev) == set(bound)
    failed, worst = [], {}
    for k, d in dev.items():
        kind, _, name = k.partition("/")
        if kind in ("grad_l2", "grad_max") and D.zero_gradient(ref, name):
            # compare_step's rule: torch has rounding noise here, this path an exact zero or noise
            if float(np.abs(upd["grads"][name]).max()) > 1e-4 * max(1.0, ref["grad_norm"]):
                failed.append((k, float(np.abs(upd["grads"][name]).max()), "zero-gradient rule"))
            continue
        frac = d / bound[k]
        if frac > worst.get(kind, (0.0, ""))[0]:
            worst[kind] = (frac, name)
        if not d <= bound[k]:
            failed.append((k, d, bound[k], round(frac, 2)))
    print(f"CONDITIONED {D.case_tag(*case)} {form}: " + ", ".join(f"{kind} {f:.2f} ({name})" if name else f"{kind} {f:.2f}"
                                                                   for kind, (f, name) in sorted(worst.items())))
    assert not failed, failed
