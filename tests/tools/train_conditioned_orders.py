#!/usr/bin/env python3
"""CPU emulations of summation orders other than torch's, on the conditioned training cases (profiles/NOTES_train_conditioned.md,
finding 2).  Not a test: prints, per case, the deviation from the float64 oracle as a multiple of the fixture's yardstick.

  chain   : the float32 step with every encoder conv's FORWARD summed as lgt_conv_kernel sums it: one float32 accumulator per
            output element that takes the 9 * CI products one after the other (chunks of 16 input channels, tap-major inside a
            chunk), bias added last.  torch's CPU conv keeps vector lanes of partial sums.  The backward is torch's.
  permute : the float32 oracle on the batch in another sample order (the same step mathematically; BatchNorm statistics,
            weight gradients and the loss add up in another order).

usage: python tests/tools/train_conditioned_orders.py [case tag ...]"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import lg_oracle as O  # noqa: E402
from tests import train_decisions_ref as D  # noqa: E402

KCT = 16


class ChainConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, b):
        ctx.save_for_backward(h, w)
        n, ci, hh, ww = h.shape
        cols = F.unfold(h, 3, padding=1).reshape(n, ci, 9, hh * ww)
        wk = w.reshape(w.shape[0], ci, 9)
        acc = torch.zeros(n, w.shape[0], hh * ww, dtype=h.dtype)
        for c0 in range(0, ci, KCT):
            for tap in range(9):
                for c in range(c0, min(ci, c0 + KCT)):
                    acc += wk[:, c, tap][None, :, None] * cols[:, c, tap][:, None, :]
        return (acc + b[None, :, None]).reshape(n, -1, hh, ww)

    @staticmethod
    def backward(ctx, dy):
        h, w = ctx.saved_tensors
        return (torch.nn.grad.conv2d_input(h.shape, w, dy, padding=1), torch.nn.grad.conv2d_weight(h, w.shape, dy, padding=1),
                dy.sum(dim=(0, 2, 3)))


def chain_conv(h, w, b, padding):
    return ChainConv.apply(h, w, b)


def result_like_oracle(r, ref, params):
    """D.step's result in cnn_train_step's layout: gradient norm in float64 from the float32 gradients as the oracle does, first
    Adam moments in float32 from them (clip coefficient, weight decay)."""
    gn = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in r["grads"].values())))
    hp = D.HPARAMS
    coef = np.float32(min(hp["max_grad_norm"] / (gn + 1e-6), 1.0))
    gp = {k: g.astype(np.float32) * coef + np.float32(hp["weight_decay"]) * params[k] for k, g in r["grads"].items()}
    return {"loss": r["loss"], "logits": r["logits"], "grad_norm": gn, "grads": r["grads"], "params": r["buffers"],
            "opt_state": {"exp_avg": {k: np.float32(1.0 - hp["betas"][0]) * g for k, g in gp.items()},
                          "exp_avg_sq": {k: np.float32(1.0 - hp["betas"][1]) * g * g for k, g in gp.items()}}}


def multiples(q, yard, floor, ref):
    out = {}
    for k, v in q.items():
        kind, _, name = k.partition("/")
        if kind in ("grad_l2", "grad_max") and D.zero_gradient(ref, name):
            continue
        cls = k if k in D.HEAD_QUANTITIES or name in D.head_tensors(ref) else kind + "/other"
        out[cls] = max(out.get(cls, 0.0), v / max(yard[k], floor[k] / 4.0))
    return out


def main():
    fx = np.load(D.FIXTURE)
    tags = sys.argv[1:] or [D.case_tag(*c) for c in D.CASES]
    for case in D.CASES:
        tag = D.case_tag(*case)
        if tag not in tags:
            continue
        params, x, y, mk = D.conditioned_inputs(fx, *case)
        ref = D.oracle_step(O, params, x, y, mk, torch.float64)
        yard = dict(zip((str(k) for k in fx[f"{tag}_yard_key"]), (float(v) for v in fx[f"{tag}_yard"])))
        floor = D.floors(ref)
        ops = {f"conv:encoder.{b}.{k}": chain_conv for b in range(len(case[1])) for k in (0, 3)}
        r = D.step(params, x, y, mk, dtype=torch.float32, ops=ops)
        chain = multiples(D.yardstick_quantities(result_like_oracle(r, ref, params), ref), yard, floor, ref)
        perm_worst = {}
        rng = np.random.default_rng(0)
        for _ in range(6):
            perm = rng.permutation(len(x))
            rp = D.oracle_step(O, params, x[perm], y[perm], [m[perm] for m in mk], torch.float32)
            rp["logits"] = rp["logits"][np.argsort(perm)]
            for k, v in multiples(D.yardstick_quantities(rp, ref), yard, floor, ref).items():
                perm_worst[k] = max(perm_worst.get(k, 0.0), v)
        print(tag)
        for k in sorted(chain):
            print(f"  {k:40s} chain {chain[k]:6.2f} x yardstick   permute {perm_worst[k]:6.2f} x", flush=True)


if __name__ == "__main__":
    main()
