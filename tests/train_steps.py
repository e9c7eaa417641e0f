"""Helpers shared by the trainer's GPU test files: whole-state snapshots, bit-for-bit comparison, the optimizer-only call
and a start state with non-trivial Adam moments.  Everything goes through GraspTrainer and the existing C-ABI."""
import ctypes as C

import numpy as np
import torch

STATE_KEYS = ("params", "buffers", "exp_avg", "exp_avg_sq", "grads")


def snapshot(tr):
    """Everything a step leaves behind: flat parameters, running statistics, both Adam moments, gradients, step count."""
    return tr._get(params=True, buffers=True, m=True, v=True, grads=True)


def assert_bits(a, b, what):
    """Bit equality of two float32 arrays (or scalars): -0.0 != +0.0, and a NaN equals only the same NaN."""
    a = np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)
    b = np.ascontiguousarray(np.asarray(b, np.float32)).reshape(-1).view(np.uint32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (f"{what}: {bad.size} of {a.size} entries differ, first at {int(bad[0])}: "
                           f"{a[bad[:1]].view(np.float32)[0]!r} vs {b[bad[:1]].view(np.float32)[0]!r}")


def assert_same_state(a, b, what):
    """a, b: snapshot() dicts."""
    assert a["step"] == b["step"], (what, a["step"], b["step"])
    for k in STATE_KEYS:
        assert_bits(a[k], b[k], f"{what}: {k}")


def assert_same_outputs(oa, ob, what):
    """oa, ob: (loss, logits, grad_norm) of train_step(..., return_logits=True)."""
    assert_bits(oa[0], ob[0], f"{what}: loss")
    assert_bits(oa[1].cpu().numpy(), ob[1].cpu().numpy(), f"{what}: logits")
    assert_bits(oa[2], ob[2], f"{what}: gradient norm")


def apply_only(tr):
    """lg_train_apply on the gradient vector as it stands (the second half of train_step_ddp).  Returns the norm."""
    from leafgrasp_amd._lib import lib
    torch.cuda.synchronize(tr.device)      # the library works on its own stream
    norm = C.c_float()
    tr._check(lib.lg_train_apply(tr._h, C.byref(tr.hp), C.byref(norm)), "lg_train_apply")
    return norm.value


def start_moments(params, names, seed):
    """Adam moments a run could have left: exp_avg of the parameters' own scale and either sign, exp_avg_sq positive."""
    rng = np.random.default_rng(seed)
    m = {k: (1e-2 * rng.standard_normal(params[k].shape)).astype(np.float32) for k in names}
    v = {k: (1e-4 * rng.random(params[k].shape) + 1e-8).astype(np.float32) for k in names}
    return m, v


def load_from_snapshot(tr, snap):
    """Put a snapshot()'s parameters, running statistics, moments and step count into another trainer of the same model."""
    sd = tr._unflat(snap["params"], tr._params)
    sd.update(tr._unflat(snap["buffers"], tr._buffers))
    tr.load_state_dict(sd, {"exp_avg": tr._unflat(snap["exp_avg"], tr._params),
                            "exp_avg_sq": tr._unflat(snap["exp_avg_sq"], tr._params), "step": snap["step"]})
