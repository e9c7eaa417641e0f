#!/usr/bin/env python3
"""The training epoch: a train_step() per batch against one train_epoch() call, in one process.

  (a) the bare inner loop, 1024 samples drawn with replacement, batch 16, 64 steps:
        steps_as_fit   what fit() does per batch: torch indexing, train_step(return_logits=True), the accuracy's .item()
        steps_only     train_step() on batches gathered beforehand, loss only
        device_epoch   one train_epoch() on the whole set and the drawn indices
  (b) one fit() epoch, 1024 training + 256 validation samples, device_eval=True, device_epoch False / True

Every timed call ends in a synchronise; host clock; routes alternate inside one loop after a warm-up; medians of --reps
(default 20) with the minimum and maximum as the spread.  The per-step routes are the reference for the time: the device
epoch passes when its median is not above a per-step median by more than that route's own min-max spread (exit status 1
otherwise).  One JSON line per case goes to --out.

    python tools/epoch_bench.py --out profiles/device_epoch_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import synthetic_inputs as S  # noqa: E402
from leafgrasp_amd.trainer import GraspTrainer  # noqa: E402

DEV = torch.device("cuda:0")
BATCH = 16


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(routes, reps, warmup):
    """routes: {name: callable}.  -> {name: [ms] * reps}, the routes taking turns."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    out = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            out[k].append(timed(fn))
    return out


def row(case, times, reference, candidate, **extra):
    r = {"case": case, **extra}
    for k, v in times.items():
        r[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}
    ref, cand = times[reference], statistics.median(times[candidate])
    r["speedup"] = round(statistics.median(ref) / cand, 3)
    r["reference_spread_ms"] = round(max(ref) - min(ref), 4)
    r["not_slower"] = bool(cand <= statistics.median(ref) + (max(ref) - min(ref)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    rng = np.random.default_rng(0)

    n, m = 1280, 1024
    fx = S.synthetic_patches(n, seed=41)
    fy = (rng.random(n) < 0.5).astype(np.float32)
    fx[fy == 1, 2] += 0.8

    # (a) the inner loop alone; one trainer per route, all from the same weights
    x, y = torch.from_numpy(fx[:m]).to(DEV), torch.from_numpy(fy[:m]).to(DEV)
    idx = torch.from_numpy(rng.integers(0, m, size=m).astype(np.int64))
    idx_dev, idx_np = idx.to(DEV), idx.numpy().astype(np.int32)
    batches = [(x[idx_dev[s:s + BATCH]], y[idx_dev[s:s + BATCH]]) for s in range(0, m, BATCH)]
    trs = {k: GraspTrainer(DEV, max_batch=BATCH, seed=7) for k in ("steps_as_fit", "steps_only", "device_epoch")}

    def steps_as_fit():
        tr, correct = trs["steps_as_fit"], 0
        for s in range(0, m, BATCH):
            bi = idx_dev[s:s + BATCH]
            _, logits, _ = tr.train_step(x[bi], y[bi], return_logits=True)
            correct += ((torch.sigmoid(logits) > 0.5).float() == y[bi]).sum().item()

    def steps_only():
        tr = trs["steps_only"]
        for bx, by in batches:
            tr.train_step(bx, by)

    def device_epoch():
        trs["device_epoch"].train_epoch(x, y, idx_np, BATCH)

    t = alternate({"steps_as_fit": steps_as_fit, "steps_only": steps_only, "device_epoch": device_epoch}, args.reps, args.warmup)
    sds = [tr.state_dict() for tr in trs.values()]
    same = all(torch.equal(sds[0][k], sd[k]) for sd in sds[1:] for k in sds[0])
    rows.append(row("inner_loop_64_steps", t, "steps_as_fit", "device_epoch", steps=m // BATCH, batch=BATCH,
                    weights_bit_equal=same))
    r2 = row("inner_loop_64_steps_vs_steps_only", {k: t[k] for k in ("steps_only", "device_epoch")}, "steps_only", "device_epoch")
    rows.append(r2)

    # (b) one fit() epoch
    fit_trs = {False: GraspTrainer(DEV, max_batch=BATCH, seed=7), True: GraspTrainer(DEV, max_batch=BATCH, seed=7)}

    def epoch(dev_epoch):
        return lambda: fit_trs[dev_epoch].fit(fx, fy, num_epochs=1, batch_size=BATCH, val_fraction=0.2, log=None,
                                              device_eval=True, device_epoch=dev_epoch)

    t = alternate({"step_loop": epoch(False), "device_epoch": epoch(True)}, args.reps, 1)
    rows.append(row("fit_epoch_1024_256", t, "step_loop", "device_epoch", train_samples=1024, val_samples=256))

    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0 if all(r["not_slower"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
