#!/usr/bin/env python3
"""tests/golden/train_conditioned.npz: first training steps whose every ReLU / max-pool decision is clear of a tie, so that
any float32 implementation takes the float64 decisions and the step can be held to float64 at rounding
(tests/test_gpu_train_conditioned.py; premises in tests/test_train_conditioned_host.py; profiles/NOTES_train_conditioned.md).

Per case of tests/train_decisions_ref.py::CASES, from synthetic_inputs.cnn_closed_form_params / synthetic_patches and seeded
keep masks, the network is walked from the input to the logits.  In every channel with a site closer to its tie than tau, the
channel's BatchNorm bias -- and in front of a pool one conv weight of the channel, for the channel-attention MLP the 1 x 1
conv bias -- is moved in float32 by a seeded random walk in steps of +-1e-3 (never beyond +-1e-2) until the channel is
clear; the next layer is walked only then (a nudge changes later layers only).  Margins are float64 values computed from the
float32 parameter values the device will be given.

tau is measured: per site group TAU_FACTOR x the largest |float32 - float64| of the oracle's forward over the sites within
1e-3 of the tie (train_decisions_ref.local_deviation), the maximum over 1, 2 and 8 threads, before and after conditioning.
TAU_FACTOR = 64 is the assumption that the device's summation order deviates from float64 by no more than a small multiple
of what torch's float32 does.

Stored (data only, no parameter tensors): per case the nudges (tensor name, flat index, delta), per site group tau, the local
deviation, the smallest margin reached and the tries, and the yardsticks: the deviation of the float32 oracle step from the
float64 oracle step on the conditioned case per quantity and tensor (train_decisions_ref.yardstick_quantities), the maximum
over 1, 2 and 8 threads.  Runs anywhere (no reference project needed): python tests/golden/make_golden_train_conditioned.py"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import lg_oracle as O  # noqa: E402
from tests import train_decisions_ref as D  # noqa: E402

TAU_FACTOR = 64.0
THREADS = (1, 2, 8)
STEP, KMAX = 1e-3, 10          # nudges are k * 1e-3, |k| <= 10
SLACK = 1.05                   # the walk clears to 1.05 tau: float64 sums of another host differ in the last bits
EPS = 1e-5
DT = torch.float64


def measure_deviation(params, x, y, mk):
    r64 = D.step(params, x, y, mk, want_grads=False)
    dev = {}
    for t in THREADS:
        torch.set_num_threads(t)
        d = D.local_deviation(D.step(params, x, y, mk, dtype=torch.float32, want_grads=False), r64)
        dev = {k: max(v, dev.get(k, 0.0)) for k, v in d.items()}
    torch.set_num_threads(THREADS[-1])
    return dev, D.margins(r64)


class Walk:
    """Nudges as integer multiples of STEP per (tensor, flat index), always applied to the ORIGINAL float32 value."""

    def __init__(self, params, seed):
        self.orig = params
        self.k = {}
        self.rng = np.random.default_rng(seed)
        self.tries = {}

    def value(self, name, idx):
        return np.float32(self.orig[name].reshape(-1)[idx] + np.float32(self.k.get((name, idx), 0) * STEP))

    def move(self, name, idx):
        k, s = self.k.get((name, idx), 0), int(self.rng.choice((-1, 1)))
        self.k[(name, idx)] = k + s if abs(k + s) <= KMAX else k - s

    def tensor(self, name):
        out = self.orig[name].copy()
        for (nm, idx), _ in self.k.items():
            if nm == name:
                out.reshape(-1)[idx] = self.value(nm, idx)
        return torch.from_numpy(out).to(DT)

    def params(self):
        names = [nm for (nm, _), k in self.k.items() if k]
        index = [idx for (_, idx), k in self.k.items() if k]
        delta = [np.float32(k * STEP) for k in self.k.values() if k]
        return names, index, delta


def normalise(o):
    """Train-mode BatchNorm without its affine part, per channel (dim 1), float64."""
    dims = [d for d in range(o.dim()) if d != 1]
    mean = o.mean(dim=dims, keepdim=True)
    var = o.var(dim=dims, unbiased=False, keepdim=True)
    return (o - mean) / torch.sqrt(var + EPS)


def clear_bn_layer(w, tau, h_in, conv, bn, pool_group, group, linear=False):
    """Walk one conv / linear + BatchNorm + ReLU (+ pool) layer until every channel is clear; returns the layer's output."""
    W, b = w.tensor(conv + ".weight"), w.tensor(conv + ".bias")
    out = F.linear(h_in, W, b) if linear else F.conv2d(h_in, W, b, padding=1)
    gamma = w.tensor(bn + ".weight")
    per = W[0].numel()
    t_relu, t_pool = SLACK * tau[group], SLACK * tau.get(pool_group, 0.0)
    zs = []
    for c in range(out.shape[1]):
        o_c, widx, n_try, mine = out[:, c:c + 1], None, 0, []
        while True:
            beta = float(w.value(bn + ".bias", c))
            z = normalise(o_c) * gamma[c] + beta
            ok_relu = float(z.abs().min()) >= t_relu
            ok_pool = pool_group is None or float(D.pool_gap(F.relu(z)).min()) >= t_pool
            if ok_relu and ok_pool:
                break
            n_try += 1
            assert n_try < 2000, (group, c)
            w.move(bn + ".bias", c)
            if not ok_pool:          # a bias moves all four entries of a cell alike: the gap needs the conv output itself
                if widx is not None and n_try % 25 == 0:      # this weight does not move the cell (a dead input): take another
                    w.k[(conv + ".weight", widx)] = 0
                    widx = None
                if widx is None:
                    widx = c * per + int(w.rng.integers(per))
                    mine.append(widx)
                w.move(conv + ".weight", widx)
                Wc = W[c:c + 1].clone()
                for i in mine:
                    Wc.reshape(-1)[i - c * per] = float(w.value(conv + ".weight", i))
                o_c = F.conv2d(h_in, Wc, b[c:c + 1], padding=1)
        w.tries[group] = w.tries.get(group, 0) + n_try
        zs.append(z)
    return F.relu(torch.cat(zs, dim=1))


def condition(w, tau, x, mk):
    p = w.orig
    h = torch.from_numpy(x).to(DT)
    nb = 0
    while f"encoder.{nb}.0.weight" in p:
        nb += 1
    mi = 0
    with torch.no_grad():
        for b in range(nb):
            h = clear_bn_layer(w, tau, h, f"encoder.{b}.0", f"encoder.{b}.1", None, f"encoder.{b}.1")
            h = clear_bn_layer(w, tau, h, f"encoder.{b}.3", f"encoder.{b}.4", f"pool.{b}", f"encoder.{b}.4")
            h = F.max_pool2d(h, 2) * torch.from_numpy(mk[mi]).to(DT)[:, :, None, None]
            mi += 1

        def chan(prefix):
            g = h.mean(dim=(2, 3), keepdim=True)
            W1 = w.tensor(prefix + ".1.weight")
            lin = F.conv2d(g, W1)
            group, n_try = prefix + ".1", 0
            for j in range(W1.shape[0]):
                while float((lin[:, j] + float(w.value(prefix + ".1.bias", j))).abs().min()) < SLACK * tau[group]:
                    n_try += 1
                    assert n_try < 2000, group
                    w.move(prefix + ".1.bias", j)
            w.tries[group] = w.tries.get(group, 0) + n_try
            a = F.relu(lin + w.tensor(prefix + ".1.bias")[None, :, None, None])
            return torch.sigmoid(F.conv2d(a, w.tensor(prefix + ".3.weight"), w.tensor(prefix + ".3.bias")))

        if "attention.0.weight" in p:
            h = h * torch.sigmoid(F.conv2d(h, w.tensor("attention.0.weight"), w.tensor("attention.0.bias")))
        elif "attention.1.weight" in p:
            h = h * chan("attention")
        elif "spatial_attention.0.weight" in p:
            sp = torch.sigmoid(F.conv2d(h, w.tensor("spatial_attention.0.weight"), w.tensor("spatial_attention.0.bias")))
            h = h * sp * chan("channel_attention")
        h = h.mean(dim=(2, 3))
        for idx in (0, 4, 8):
            h = clear_bn_layer(w, tau, h, f"classifier.{idx}", f"classifier.{idx + 1}", None, f"classifier.{idx + 1}", linear=True)
            h = h * torch.from_numpy(mk[mi]).to(DT)
            mi += 1


def main():
    out = {"tau_factor": np.array(TAU_FACTOR), "threads": np.array(THREADS)}
    for case in D.CASES:
        t0 = time.time()
        tag = D.case_tag(*case)
        params, x, y, mk = D.case_inputs(*case)
        groups = D.site_groups(params)
        dev0, margin0 = measure_deviation(params, x, y, mk)
        tau = {k: TAU_FACTOR * dev0[k] for k in groups}
        w = Walk(params, 1000 + D.case_seed(*case))
        for rnd in range(6):
            condition(w, tau, x, mk)
            nudged = D.apply_nudges(params, *w.params())
            dev, margin = measure_deviation(nudged, x, y, mk)
            tau = {k: max(tau[k], TAU_FACTOR * dev[k]) for k in groups}
            if all(margin[k] >= tau[k] for k in groups):
                break
        else:
            raise SystemExit(f"{tag}: margins and tau did not settle")
        names, index, delta = w.params()
        assert max(abs(float(d)) for d in delta) <= 1e-2 + 1e-9
        out[f"{tag}_nudge_name"], out[f"{tag}_nudge_index"] = np.array(names), np.array(index, np.int64)
        out[f"{tag}_nudge_delta"] = np.array(delta, np.float32)
        out[f"{tag}_group"] = np.array(groups)
        out[f"{tag}_tau"] = np.array([tau[k] for k in groups])
        out[f"{tag}_dev"] = np.array([dev[k] for k in groups])
        out[f"{tag}_dev_before"] = np.array([dev0[k] for k in groups])
        out[f"{tag}_margin"] = np.array([margin[k] for k in groups])
        out[f"{tag}_margin_before"] = np.array([margin0[k] for k in groups])
        out[f"{tag}_tries"] = np.array([w.tries.get(k, 0) for k in groups], np.int64)
        ref = D.oracle_step(O, nudged, x, y, mk, torch.float64)
        yard = {}
        for t in THREADS:
            torch.set_num_threads(t)
            q = D.yardstick_quantities(D.oracle_step(O, nudged, x, y, mk, torch.float32), ref)
            yard = {k: max(v, yard.get(k, 0.0)) for k, v in q.items()}
        torch.set_num_threads(THREADS[-1])
        out[f"{tag}_yard_key"], out[f"{tag}_yard"] = np.array(list(yard)), np.array(list(yard.values()))
        enc = [v for k, v in yard.items() if k.startswith("grad_l2/encoder") and not D.zero_gradient(ref, k[8:])]
        cls = [v for k, v in yard.items() if k.startswith("grad_l2/classifier") and not D.zero_gradient(ref, k[8:])]
        print(f"{tag}: {len(names)} nudges, {sum(w.tries.values())} tries, {rnd + 1} round(s), tau {min(tau.values()):.1e} .. "
              f"{max(tau.values()):.1e}, smallest margin / tau {min(margin[k] / tau[k] for k in groups):.2f}, yardstick grad L2 encoder "
              f"{min(enc):.1e} .. {max(enc):.1e} classifier {min(cls):.1e} .. {max(cls):.1e}, {time.time() - t0:.1f} s", flush=True)
    np.savez_compressed(D.FIXTURE, **out)
    print("wrote", D.FIXTURE, os.path.getsize(D.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
