"""Device-drawn dropout masks (lgt_mask_kernel, masks=None -- the only way training calls the step) against the restated
draw of tests/train_masks_ref.py.  Trainer A steps with masks=None; trainer B starts from the same state and is handed
train_masks_ref.masks(seed, step, N, layout).  Only the origin of the mask buffer differs and every reduction of the step
is ordered (test_gradients_only_and_determinism), so A and B must agree bit for bit on loss, logits, gradient norm, every
gradient, parameters, both Adam moments and the running statistics."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import synthetic_inputs as S  # noqa: E402
from tests import train_masks_ref as R  # noqa: E402
from tests.test_gpu_train import ENCODERS, make_trainer  # noqa: E402
from tests.train_steps import apply_only, assert_bits, assert_same_outputs, assert_same_state, snapshot, start_moments  # noqa: E402

SMALL = (32, 64, 128)
BIG_SEED = (1 << 33) + 12345          # seed * 0x100000001B3 wraps in 64 bits


def run_pair(att, filt, n, seed, script, start_step=0):
    """script: a sequence of "update" (train_step), "grads" (train_step, apply_update=False) and "apply" (lg_train_apply).
    `counter` is the device's step count as the header defines it: what the next drawn mask is seeded with."""
    from leafgrasp_amd.trainer import dropout_layout, parameter_layout
    lay = dropout_layout(filt)
    params = S.cnn_closed_form_params(seed=11, attention_type=att, filters=filt)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    opt = None
    if start_step:
        m, v = start_moments(params, [k for k, _ in parameter_layout(filt, att)[0]], 3)
        opt = {"exp_avg": m, "exp_avg_sq": v, "step": start_step}
    a, b = make_trainer(att, filt, 16, seed=seed), make_trainer(att, filt, 16, seed=seed)
    a.load_state_dict(sd, opt)
    b.load_state_dict(sd, opt)
    counter, outs = start_step, []
    for i, what in enumerate(script):
        tag = f"{what} #{i} (device step count {counter})"
        if what == "apply":
            assert_bits(apply_only(a), apply_only(b), tag + ": norm")
            counter += 1
        else:
            x = S.synthetic_patches(n, seed=60 + i)
            y = ((np.arange(n) + i) % 3 == 0).astype(np.float32)
            upd = what == "update"
            oa = a.train_step(x, y, masks=None, apply_update=upd, return_logits=True)
            ob = b.train_step(x, y, masks=R.masks(seed, counter, n, lay), apply_update=upd, return_logits=True)
            assert_same_outputs(oa, ob, tag)
            outs.append(oa)
            counter += int(upd)
        sa = snapshot(a)
        assert sa["step"] == counter
        assert_same_state(sa, snapshot(b), tag)
    return outs


@pytest.mark.parametrize("att,filt", ENCODERS, ids=["standard", "lightweight", "wide", "deep"])
def test_three_updating_steps_every_encoder(att, filt):
    """The device step counter advances 0 -> 1 -> 2; 13 samples (ragged against every tile of the step)."""
    run_pair(att, filt, 13, 42, ["update"] * 3)


@pytest.mark.parametrize("att", ["spatial", "channel", "hybrid", "none"])
def test_every_attention_type(att):
    run_pair(att, SMALL, 16, 42, ["update"] * 2)


@pytest.mark.parametrize("filt", [SMALL, (64, 128, 256)], ids=["lightweight", "standard"])
@pytest.mark.parametrize("n", [2, 16])
def test_batch_sizes(n, filt):
    """With 13 above: the smallest batch the library accepts, an odd one, and max_batch."""
    run_pair("spatial", filt, n, 42, ["update"] * 3)


@pytest.mark.parametrize("seed", [7, BIG_SEED])
@pytest.mark.parametrize("filt", [SMALL, (64, 128, 256)], ids=["lightweight", "standard"])
def test_seeds(seed, filt):
    run_pair("spatial", filt, 13, seed, ["update"] * 2)


@pytest.mark.parametrize("filt", [SMALL, (64, 128, 256)], ids=["lightweight", "standard"])
def test_step_count_from_loaded_optimizer_state(filt):
    """load_state_dict(..., optimizer_state={..., "step": 7}): the counter comes from lg_train_set_state."""
    run_pair("spatial", filt, 13, 42, ["update"] * 2, start_step=7)


@pytest.mark.parametrize("filt", [SMALL, (64, 128, 256)], ids=["lightweight", "standard"])
def test_gradients_only_twice_draws_the_same_masks(filt):
    """apply_update=False does not advance the counter: two such steps on the same batch draw the masks of the same step."""
    from leafgrasp_amd.trainer import dropout_layout
    n, seed = 16, 42
    x, y = S.synthetic_patches(n, seed=61), (np.arange(n) % 3 == 0).astype(np.float32)
    params = S.cnn_closed_form_params(seed=11, attention_type="spatial", filters=filt)
    a, b = make_trainer("spatial", filt, 16, seed=seed), make_trainer("spatial", filt, 16, seed=seed)
    for t in (a, b):
        t.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    o1 = a.train_step(x, y, apply_update=False, return_logits=True)
    g1 = snapshot(a)
    o2 = a.train_step(x, y, apply_update=False, return_logits=True)
    g2 = snapshot(a)
    ob = b.train_step(x, y, masks=R.masks(seed, 0, n, dropout_layout(filt)), apply_update=False, return_logits=True)
    # (the running statistics moved between the two forwards, as in a train-mode forward; the outputs do not read them)
    assert_same_outputs(o1, o2, "first and second gradients-only step")
    assert_same_outputs(o1, ob, "drawn and given masks of step 0")
    for k in ("params", "exp_avg", "exp_avg_sq", "grads"):
        assert_bits(g1[k], g2[k], k)
    assert_same_state(g1, snapshot(b), "after one gradients-only step")
    assert g2["step"] == 0


@pytest.mark.parametrize("filt", [SMALL, (64, 128, 256)], ids=["lightweight", "standard"])
def test_data_parallel_order_on_one_process(filt):
    """train_step(apply_update=False), lg_train_apply, next step: lg_train_apply advances the counter, so the next step
    draws the masks of the next step number."""
    outs = run_pair("spatial", filt, 13, 42, ["grads", "apply", "grads", "apply", "update"])
    assert len(outs) == 3
