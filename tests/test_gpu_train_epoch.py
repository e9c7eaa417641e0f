"""lg_train_epoch / GraspTrainer.train_epoch: the steps of one epoch enqueued in one call, batches gathered on the device.
The reference in every case is the per-step route: a second trainer with the same initial state and seed driven by
train_step on x[idx[k*b:(k+1)*b]].  Nothing in the epoch changes the order of any sum, so the state after it (parameters,
running statistics, Adam moments, gradients, step count) and the per-step losses, gradient norms and logits are compared
bit for bit.  `correct` is compared with fit()'s expression on those logits; the library counts logit > 0 where fit()
writes sigmoid(logit) > 0.5 in float32, which differ only for 0 < logit <~ 1.2e-7, so each case first asserts that none of
its logits lies within 1e-6 of zero."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import synthetic_inputs as S  # noqa: E402
from tests.test_gpu_train import DEV, make_trainer  # noqa: E402
from tests.test_gpu_train_modes import trainer_in_mode  # noqa: E402
from tests.train_steps import assert_bits, assert_same_state, snapshot  # noqa: E402

STANDARD = ("spatial", (64, 128, 256))
SEED = 42
N_SET = 23
SENTINEL = 12345.0
_FP = C.POINTER(C.c_float)


def training_set(n=N_SET, seed=61):
    x = torch.from_numpy(S.synthetic_patches(n, seed=seed)).to(DEV)
    y = torch.from_numpy(((np.arange(n) * 7 + seed) % 3 == 0).astype(np.float32)).to(DEV)
    return x, y


def new_trainer(att, filt, monkeypatch=None, mode="default"):
    tr = trainer_in_mode(monkeypatch, mode, att, filt, 16) if mode != "default" else make_trainer(att, filt, 16, seed=SEED)
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in S.cnn_closed_form_params(seed=12, attention_type=att, filters=filt).items()})
    return tr


def draw(m, seed, n=N_SET):
    return np.random.default_rng(seed).integers(0, n, size=m).astype(np.int32)


def by_steps(tr, x, y, idx, batch):
    """fit()'s inner loop on train_step.  Returns what train_epoch returns, `correct` by fit()'s own expression."""
    losses, norms, logits, correct = [], [], [], 0
    for s in range(0, len(idx), batch):
        bi = torch.from_numpy(np.asarray(idx[s:s + batch], np.int64)).to(DEV)
        if bi.numel() < 2:
            continue
        loss, lg, gn = tr.train_step(x[bi], y[bi], return_logits=True)
        losses.append(loss)
        norms.append(gn)
        logits.append(lg.cpu().numpy())
        correct += ((torch.sigmoid(lg) > 0.5).float() == y[bi]).sum().item()
    logits = np.concatenate(logits) if logits else np.zeros(0, np.float32)
    assert logits.size == 0 or np.abs(logits).min() >= 1e-6, "a logit within 1e-6 of zero: choose another seed for this case"
    return {"losses": np.asarray(losses, np.float32), "grad_norms": np.asarray(norms, np.float32), "logits": logits,
            "correct": int(correct), "n_steps": len(losses)}


def assert_same_epoch(ep, ref, what):
    """ep: train_epoch(..., return_logits=True); ref: by_steps()."""
    used = ref["logits"].size
    assert ep["n_steps"] == ref["n_steps"], what
    assert ep["losses"].dtype == np.float32 and ep["losses"].shape == (ref["n_steps"],), what
    assert_bits(ep["losses"], ref["losses"], f"{what}: losses")
    assert_bits(ep["grad_norms"], ref["grad_norms"], f"{what}: gradient norms")
    got = ep["logits"].cpu().numpy()
    assert_bits(got[:used], ref["logits"], f"{what}: logits")
    assert np.isnan(got[used:]).all(), f"{what}: the skipped tail's logits"
    assert ep["correct"] == ref["correct"], what


def compare_routes(att, filt, idx, batch, what, monkeypatch=None, mode="default"):
    x, y = training_set()
    a, b = new_trainer(att, filt, monkeypatch, mode), new_trainer(att, filt)
    ep = a.train_epoch(x, y, idx, batch, return_logits=True)
    ref = by_steps(b, x, y, idx, batch)
    assert_same_epoch(ep, ref, what)
    assert_same_state(snapshot(a), snapshot(b), what)
    assert snapshot(a)["step"] == ref["n_steps"] and a.num_batches_tracked == b.num_batches_tracked == ref["n_steps"]
    for k, v in a.state_dict().items():
        assert_bits(v.numpy(), b.state_dict()[k].numpy(), f"{what}: state_dict {k}")
    return ep


def raw_epoch(tr, x, y, idx, batch, logits=None):
    """lg_train_epoch itself.  Returns (status, n_steps, losses)."""
    from leafgrasp_amd._lib import lib
    idx = np.ascontiguousarray(idx, np.int32)
    losses = np.full(len(idx) // 2 + 1, SENTINEL, np.float32)
    n_steps = C.c_int32(-7)
    torch.cuda.synchronize()
    rc = lib.lg_train_epoch(tr._h, x.data_ptr(), y.data_ptr(), y.shape[0], idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx),
                            batch, tr.seed, C.byref(tr.hp), losses.ctypes.data_as(_FP), None, None,
                            logits.data_ptr() if logits is not None else None, C.byref(n_steps))
    return rc, n_steps.value, losses


@pytest.mark.parametrize("batch,m", [(4, 19), (4, 17), (2, 7), (16, 40)], ids=["tail-3", "tail-1-skipped", "batch-2", "max-batch"])
def test_epoch_equals_its_steps(batch, m):
    """4 / 19: every BatchNorm reduction in one chunk, the tail of 3 used.  4 / 17: the tail of 1 skipped.  2 / 7: the smallest
    batch.  16 / 40: BatchNorm in sample chunks on the first layers, a tail of 8."""
    ep = compare_routes(*STANDARD, draw(m, 100 + m), batch, f"batch {batch}, m {m}")
    assert ep["n_steps"] == m // batch + (m % batch >= 2)


def test_skipped_tail_leaves_its_logit_alone():
    x, y = training_set()
    idx = draw(17, 117)
    a, b = new_trainer(*STANDARD), new_trainer(*STANDARD)
    logits = torch.full((17,), SENTINEL, dtype=torch.float32, device=DEV)
    rc, n_steps, losses = raw_epoch(a, x, y, idx, 4, logits)
    ref = by_steps(b, x, y, idx, 4)
    assert rc == 0 and n_steps == 4
    got = logits.cpu().numpy()
    assert_bits(got[:16], ref["logits"], "logits")
    assert got[16] == SENTINEL
    assert_bits(losses[:4], ref["losses"], "losses")
    assert (losses[4:] == SENTINEL).all()
    assert_same_state(snapshot(a), snapshot(b), "tail of 1")


def test_repeated_and_descending_indices():
    idx = np.array([5, 5, 2, 9, 7, 7, 7, 7, 22, 21, 20, 19, 3, 2, 1, 0], np.int32)
    compare_routes(*STANDARD, idx, 4, "repeats, one-sample batch, descending")


@pytest.mark.parametrize("m", [0, 1])
def test_no_step_leaves_the_state(m):
    x, y = training_set()
    tr = new_trainer(*STANDARD)
    tr.train_step(x[:4], y[:4])   # gradients, moments and a step count worth keeping
    before = snapshot(tr)
    ep = tr.train_epoch(x, y, draw(m, 5), 4, return_logits=True)
    assert ep["n_steps"] == 0 and ep["correct"] == 0 and ep["losses"].shape == (0,) and ep["grad_norms"].shape == (0,)
    assert ep["logits"].shape == (m,) and tr.num_batches_tracked == 1
    assert_same_state(snapshot(tr), before, f"m = {m}")


@pytest.mark.parametrize("att,filt", [("hybrid", (64, 128, 256)), ("spatial", (64, 128, 256, 512))], ids=["hybrid", "four-blocks"])
def test_other_models(att, filt):
    compare_routes(att, filt, draw(10, 31), 4, f"{att} {filt}")


def test_step_epoch_step_on_one_trainer():
    x, y = training_set()
    a, b = new_trainer(*STANDARD), new_trainer(*STANDARD)
    first, idx, last = draw(5, 1), draw(11, 2), draw(3, 3)
    outs = []
    for tr in (a, b):
        o1 = by_steps(tr, x, y, first, 5)
        mid = tr.train_epoch(x, y, idx, 4, return_logits=True) if tr is a else by_steps(tr, x, y, idx, 4)
        o3 = by_steps(tr, x, y, last, 3)
        outs.append((o1, mid, o3, snapshot(tr)))
    assert_same_epoch(outs[0][1], outs[1][1], "epoch between two steps")
    for k in (0, 2):
        assert_bits(outs[0][k]["losses"], outs[1][k]["losses"], f"step {k}: loss")
        assert_bits(outs[0][k]["logits"], outs[1][k]["logits"], f"step {k}: logits")
    assert_same_state(outs[0][3], outs[1][3], "step, epoch, step")
    assert outs[0][3]["step"] == 5 and a.num_batches_tracked == b.num_batches_tracked == 5


def test_two_epochs_in_a_row():
    """The device's step counter feeds the dropout masks: the second epoch must start where the first one stopped."""
    x, y = training_set()
    a, b = new_trainer(*STANDARD), new_trainer(*STANDARD)
    for e, m in enumerate((9, 11)):
        idx = draw(m, 50 + e)
        assert_same_epoch(a.train_epoch(x, y, idx, 4, return_logits=True), by_steps(b, x, y, idx, 4), f"epoch {e}")
        assert_same_state(snapshot(a), snapshot(b), f"epoch {e}")
    assert snapshot(a)["step"] == 5


@pytest.mark.parametrize("mode", ["streams", "graph"])
def test_opt_in_modes_equal_the_default_mode_steps(monkeypatch, mode):
    """streams: the epoch honours the second stream.  graph: the epoch issues plain launches on a trainer whose steps replay
    a graph -- a step before it captures one, so the epoch runs between a capture and its replay."""
    x, y = training_set()
    a, b = new_trainer(*STANDARD, monkeypatch, mode), new_trainer(*STANDARD)
    idx = draw(19, 77)
    for tr in (a, b):
        by_steps(tr, x, y, idx[:4], 4)
    ep, ref = a.train_epoch(x, y, idx, 4, return_logits=True), by_steps(b, x, y, idx, 4)
    assert_same_epoch(ep, ref, mode)
    for tr in (a, b):
        by_steps(tr, x, y, idx[4:8], 4)
    assert_same_state(snapshot(a), snapshot(b), mode)


@pytest.mark.parametrize("bad", [-1, N_SET])
def test_index_outside_the_set_is_refused(bad):
    from leafgrasp_amd._lib import LG_ERR_INVALID
    x, y = training_set()
    tr = new_trainer(*STANDARD)
    tr.train_step(x[:4], y[:4])
    before = snapshot(tr)
    idx = draw(12, 9)
    idx[10] = bad   # in the last step: nothing of the steps in front of it may have run
    rc, n_steps, losses = raw_epoch(tr, x, y, idx, 4)
    assert rc == LG_ERR_INVALID and n_steps == -7 and (losses == SENTINEL).all()
    assert_same_state(snapshot(tr), before, f"index {bad}")
    from leafgrasp_amd._lib import LgError
    with pytest.raises(LgError, match=r"idx\[10\]"):
        tr.train_epoch(x, y, idx, 4)
    assert tr.num_batches_tracked == 1


@pytest.mark.parametrize("batch", [1, 17])
def test_batch_outside_the_trainer_is_refused(batch):
    from leafgrasp_amd._lib import LG_ERR_INVALID
    x, y = training_set()
    tr = new_trainer(*STANDARD)
    before = snapshot(tr)
    rc, n_steps, _ = raw_epoch(tr, x, y, draw(20, 4), batch)
    assert rc == LG_ERR_INVALID and n_steps == -7
    assert_same_state(snapshot(tr), before, f"batch {batch}")


@pytest.mark.parametrize("device_eval", [False, True])
def test_fit_device_epoch_equals_the_step_loop(device_eval):
    n = 40
    x = S.synthetic_patches(n, seed=40)
    y = (np.random.default_rng(0).random(n) < 0.5).astype(np.float32)
    x[y == 1, 2] += 0.8
    hist, trs = {}, {}
    for dev_epoch in (False, True):
        tr = make_trainer(*STANDARD, 16, seed=7)
        hist[dev_epoch] = tr.fit(x, y, num_epochs=2, batch_size=4, log=None, device_eval=device_eval, device_epoch=dev_epoch)
        trs[dev_epoch] = tr
    assert len(hist[True]["train_losses"]) == 2
    assert hist[True] == hist[False]
    a, b = trs[True].state_dict(), trs[False].state_dict()
    assert a.keys() == b.keys()
    for k in a:
        assert_bits(a[k].numpy(), b[k].numpy(), k)
    assert trs[True].num_batches_tracked == trs[False].num_batches_tracked == 16
    assert_same_state(snapshot(trs[True]), snapshot(trs[False]), "after fit")
