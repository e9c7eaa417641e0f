#!/usr/bin/env python3
"""What ranking every candidate costs: select_grasp_points_batch (lg_select_grasp) against select_grasp_candidates_batch
(lg_select_grasp_candidates) at 1080p with the closed-form CNN weights, B = 1, 32, 256 by default.  One JSON line per B: the
whole call between two device events on the current stream, the two calls alternating, median of `steps` each, and the
per-launch event times of lg_finish_kernel ("finish") and lg_candidates_kernel ("candidates") from lg_profile_enable.
Usage: python tools/candidates_bench.py [steps] [B ...]"""
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

H, W, N_DISTINCT = 1080, 1920, 8
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
Bs = [int(a) for a in sys.argv[2:]] or [1, 32, 256]
dev = torch.device("cuda:0")

scenes = []
for s in range(N_DISTINCT):   # the benchmark's scenes: seeds 100.., the largest leaf of each
    labels, depth, P = SI.synthetic_scene(H, W, seed=100 + s)
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    scenes.append((labels == ids[np.argmax(counts)], depth))

sel = L.GraspPointSelector(dev, load_model=False)
sel.set_camera_params(P)
sel.set_cnn_state_dict(SI.cnn_closed_form_params(seed=0))


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
    plain = lambda: sel.select_grasp_points_batch(masks, depths)           # noqa: E731
    ranked = lambda: sel.select_grasp_candidates_batch(masks, depths)      # noqa: E731
    for _ in range(3):
        plain()
        ranked()
    torch.cuda.synchronize()
    tp, tr = [], []
    for i in range(steps):   # alternate, and alternate which one goes first
        if i % 2:
            tr.append(timed(ranked))
            tp.append(timed(plain))
        else:
            tp.append(timed(plain))
            tr.append(timed(ranked))
    lib.lg_profile_enable(sel._h, 1)
    for _ in range(steps):
        ranked()
    kern = {}
    for name in ("finish", "candidates"):
        n, ms = C.c_int(0), C.c_double(0.0)
        lib.lg_profile_read(sel._h, name.encode(), C.byref(n), C.byref(ms))
        kern[name + "_ms"] = round(ms.value / max(n.value, 1), 4)
    lib.lg_profile_enable(sel._h, 0)
    mp, mr = float(np.median(tp)), float(np.median(tr))
    print(json.dumps({"B": B, "H": H, "W": W, "top_k": 20, "steps": steps, "select_ms_median": round(mp, 4),
                      "candidates_ms_median": round(mr, 4), "delta_ms": round(mr - mp, 4),
                      "select_ms_min": round(float(np.min(tp)), 4), "candidates_ms_min": round(float(np.min(tr)), 4), **kern}),
          flush=True)
