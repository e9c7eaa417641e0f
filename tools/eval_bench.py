#!/usr/bin/env python3
"""Trainer -> inference hand-off and validation: the host route against the device route, in one process.

  (a) sel.set_cnn_state_dict(tr.state_dict())      (b) sel.load_from_trainer(tr)        standard and 4-block encoder
  (c) predict_logits + the loss per 16 samples      (d) tr.evaluate                      2048 samples
  (e) one fit() epoch, 1024 training + 256 validation samples, device_eval False / True

Every timed call ends in a synchronise; host clock; routes alternate inside one loop after a warm-up; medians of --reps
(default 20) with the minimum and maximum as the spread.  One JSON line per case goes to --out.

    python tools/eval_bench.py --out profiles/device_eval_bench.jsonl
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
import leafgrasp_amd as L  # noqa: E402
import synthetic_inputs as S  # noqa: E402
from leafgrasp_amd.trainer import GraspTrainer, analyze_predictions  # noqa: E402

DEV = torch.device("cuda:0")


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


def row(case, times, **extra):
    r = {"case": case, **extra}
    for k, v in times.items():
        r[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}
    names = list(times)
    if len(names) == 2:
        r["speedup"] = round(statistics.median(times[names[0]]) / statistics.median(times[names[1]]), 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    rows = []
    rng = np.random.default_rng(0)

    for name, att, filt in (("standard", "spatial", (64, 128, 256)), ("four_block", "hybrid", (64, 128, 256, 512))):
        tr = GraspTrainer(DEV, attention_type=att, encoder_filters=filt, max_batch=16)
        sel = L.GraspPointSelector(DEV, load_model=False)
        t = alternate({"host_route": lambda: sel.set_cnn_state_dict(tr.state_dict()),
                       "device_route": lambda: sel.load_from_trainer(tr)}, args.reps, args.warmup)
        rows.append(row(f"handoff_{name}", t, encoder=list(filt), attention=att))
        # the steady state of a training loop: every hand-off after the first is an in-place refresh
        sel.load_from_trainer(tr)
        t = alternate({"device_refresh": lambda: sel.load_from_trainer(tr)}, args.reps, args.warmup)
        rows.append(row(f"refresh_{name}", t, encoder=list(filt), attention=att))
        del sel, tr

    n = 2048
    x = torch.from_numpy(S.synthetic_patches(n, seed=40)).to(DEV)
    y = torch.from_numpy((rng.random(n) < 0.5).astype(np.float32)).to(DEV)
    tr = GraspTrainer(DEV, max_batch=16)
    sel = L.GraspPointSelector(DEV, load_model=False)

    def present():
        vl = tr.predict_logits(x, selector=sel)
        vb = [tr.bce_with_logits(vl[s:s + 16], y[s:s + 16]).item() for s in range(0, n, 16)]
        return float(np.mean(vb)), analyze_predictions(vl, y)

    def device():
        ev = tr.evaluate(x, y, selector=sel, batch_size=16)
        return ev["val_loss"], ev["metrics"]

    (la, ma), (lb, mb) = present(), device()
    t = alternate({"host_route": present, "device_route": device}, args.reps, args.warmup)
    rows.append(row("validate_2048", t, samples=n, loss_host_route=la, loss_device_route=lb, metrics_equal=ma == mb))

    if not args.skip_fit:
        n = 1280
        fx = S.synthetic_patches(n, seed=41)
        fy = (rng.random(n) < 0.5).astype(np.float32)
        fx[fy == 1, 2] += 0.8
        trainers = {False: GraspTrainer(DEV, max_batch=16, seed=7), True: GraspTrainer(DEV, max_batch=16, seed=7)}

        def epoch(dev_eval):
            return lambda: trainers[dev_eval].fit(fx, fy, num_epochs=1, batch_size=16, val_fraction=0.2, log=None, device_eval=dev_eval)

        t = alternate({"host_route": epoch(False), "device_route": epoch(True)}, args.reps, 1)
        rows.append(row("fit_epoch_1024_256", t, train_samples=1024, val_samples=256))

    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
