"""CPU tests (no GPU) of the device epoch's host half: lg_train_epoch_plan -- the batching rule of GraspTrainer.fit's inner
loop as the library states it -- against a Python restatement of that loop, and the argument checks of lg_train_epoch that
answer before any device is touched."""
import ctypes as C

import pytest

from leafgrasp_amd import _lib

BATCHES = (2, 3, 16, 64)


def sizes(batch):
    return (0, 1, 2, 3, batch - 1, batch, batch + 1, 2 * batch + 1, 1000)


def fit_loop(m, batch):
    """fit(): `for s in range(0, m, batch)`, a batch of fewer than 2 samples skipped.  Returns the sizes of the steps run."""
    run = []
    for s in range(0, m, batch):
        n = min(m, s + batch) - s
        if n < 2:
            continue
        run.append(n)
    return run


def plan(m, batch):
    n_steps, last_n = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.lib.lg_train_epoch_plan(m, batch, C.byref(n_steps), C.byref(last_n))
    return rc, n_steps.value, last_n.value


@pytest.mark.parametrize("batch", BATCHES)
def test_plan_is_fits_loop(batch):
    for m in sizes(batch):
        run = fit_loop(m, batch)
        rc, n_steps, last_n = plan(m, batch)
        assert rc == _lib.LG_OK, (m, batch)
        assert n_steps == len(run), (m, batch)
        assert last_n == (run[-1] if run else 0), (m, batch)
        assert all(n == batch for n in run[:-1]), (m, batch)   # every step but the last is a full batch


def test_plan_outputs_are_optional():
    n_steps = C.c_int32(-7)
    assert _lib.lib.lg_train_epoch_plan(19, 4, C.byref(n_steps), None) == _lib.LG_OK and n_steps.value == 5
    assert _lib.lib.lg_train_epoch_plan(19, 4, None, None) == _lib.LG_OK


@pytest.mark.parametrize("m,batch", [(10, 1), (10, 0), (10, -4), (-1, 4), (2 ** 31, 4)])
def test_plan_refuses(m, batch):
    rc, n_steps, last_n = plan(m, batch)
    assert rc == _lib.LG_ERR_INVALID
    assert (n_steps, last_n) == (-7, -7)   # nothing written


def test_epoch_null_trainer_is_invalid_without_a_device():
    hp = _lib.LgTrainHparams(5e-4, 0.9, 0.999, 1e-8, 0.01, 1.0, 2.0)
    idx = (C.c_int32 * 4)(0, 1, 2, 3)
    n_steps = C.c_int32(-7)
    rc = _lib.lib.lg_train_epoch(None, 16, 16, 4, idx, 4, 2, 42, C.byref(hp), None, None, None, None, C.byref(n_steps))
    assert rc == _lib.LG_ERR_INVALID and n_steps.value == -7
