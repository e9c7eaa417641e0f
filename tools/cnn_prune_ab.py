#!/usr/bin/env python3
"""What the CNN pruning of lg_select_grasp saves and what its survivor list costs: a default handle against one created with
LG_CNN_PRUNE=0, the two alternating on the same frames at 1080p (the benchmark's scenes, closed-form CNN weights), for
  default        lg_params as they are, bool masks (traditional scores 0.75-0.94: few candidates can still win),
  halved         the four score weights halved, bool masks (traditional scores below 0.5: a candidate within 0.225 of the
                 best survives unless it lies on the border),
  quarter_uint8  the weights quartered and uint8 masks (scores below 0.25, border candidates scored: every candidate of a
                 frame whose best score is below 0.225 survives, so the difference is the price of the list, the indirection
                 and the count read on the device).
One JSON line per (B, case): the whole call between two device events, median / min of `steps`, the patches each handle put
through the CNN, per-launch event times of the kernels involved, and whether the result rows are equal byte for byte.
Usage: python tools/cnn_prune_ab.py [steps] [B ...]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import leafgrasp_amd as L  # noqa: E402
import synthetic_inputs as SI  # noqa: E402
from leafgrasp_amd._lib import lib  # noqa: E402

H, W, N_DISTINCT = 1080, 1920, 32
WEIGHTS = ("w_approach", "w_sdf", "w_flat", "w_access")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
Bs = [int(a) for a in sys.argv[2:]] or [1, 256]
dev = torch.device("cuda:0")

scenes = []
for s in range(N_DISTINCT):   # the benchmark's scenes: seeds 100.., the largest leaf of each
    labels, depth, P = SI.synthetic_scene(H, W, seed=100 + s)
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    scenes.append((labels == ids[np.argmax(counts)], depth))


def selector(prune):
    if prune:
        os.environ.pop("LG_CNN_PRUNE", None)
    else:
        os.environ["LG_CNN_PRUNE"] = "0"   # read at lg_create
    sel = L.GraspPointSelector(dev, load_model=False)
    os.environ.pop("LG_CNN_PRUNE", None)
    sel.set_camera_params(P)
    sel.set_cnn_state_dict(SI.cnn_closed_form_params(seed=0))
    return sel


sels = {"pruned": selector(True), "all": selector(False)}
defaults = {w: getattr(sels["all"].params, w) for w in WEIGHTS}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for B in Bs:
    masks = torch.from_numpy(np.stack([scenes[b % N_DISTINCT][0] for b in range(B)])).to(dev)
    depths = torch.from_numpy(np.stack([scenes[b % N_DISTINCT][1] for b in range(B)])).to(dev)
    for case, scale, as_bool in (("default", 1.0, True), ("halved", 0.5, True), ("quarter_uint8", 0.25, False)):
        mk = masks if as_bool else masks.view(torch.uint8)
        for sel in sels.values():
            for w in WEIGHTS:
                setattr(sel.params, w, defaults[w] * scale)
        run = {k: (lambda s=s: s.select_grasp_points_batch(mk, depths)) for k, s in sels.items()}
        rows, scored = {}, {}
        for k, s in sels.items():
            for _ in range(3):
                run[k]()
            rows[k] = bytes(s.last_results)
            scored[k] = s.cnn_scored()
        torch.cuda.synchronize()
        t = {"pruned": [], "all": []}
        for i in range(steps):   # alternate, and alternate which one goes first
            for k in (("pruned", "all") if i % 2 else ("all", "pruned")):
                t[k].append(timed(run[k]))
        kern = {}
        for k, s in sels.items():
            lib.lg_profile_enable(s._h, 1)
            for _ in range(steps):
                run[k]()
            for name in ("topk", "survivors", "gather", "cnn", "finish"):
                n, ms = C.c_int(0), C.c_double(0.0)
                lib.lg_profile_read(s._h, name.encode(), C.byref(n), C.byref(ms))
                kern[f"{k}_{name}_ms"] = round(ms.value / max(n.value, 1), 4)
            lib.lg_profile_enable(s._h, 0)
        print(json.dumps({"B": B, "H": H, "W": W, "case": case, "steps": steps,
                          "patches_pruned": scored["pruned"], "patches_all": scored["all"],
                          "rows_equal": rows["pruned"] == rows["all"],
                          "pruned_ms_median": round(float(np.median(t["pruned"])), 4),
                          "all_ms_median": round(float(np.median(t["all"])), 4),
                          "pruned_ms_min": round(float(np.min(t["pruned"])), 4), "all_ms_min": round(float(np.min(t["all"])), 4),
                          "pruned_ms_max": round(float(np.max(t["pruned"])), 4), "all_ms_max": round(float(np.max(t["all"])), 4),
                          **kern}), flush=True)
