#!/usr/bin/env python3
"""The per-frame serial links of select_grasp_points_batch at 1080p with the closed-form CNN weights, B = 1, 32, 256 by default:
the bit-row pass ("prep"), the window kernel ("bbox"), the greedy top-k ("topk") and the survivor list ("survivors") from the
library's own event pairs (lg_profile_enable mode 1), and the whole call between two device events.  One JSON line per B;
topk_round_us = top-k time / rounds (top_k = 20 picks per frame on these scenes).
Usage: python tools/topk_chain_bench.py [steps] [B ...]      (LG_LIB_PATH selects another build of the library)"""
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

H, W, N_DISTINCT, TOP_K = 1080, 1920, 8, 20
STAGES = ("prep", "bbox", "topk", "survivors")
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

for B in Bs:
    masks = torch.from_numpy(np.stack([scenes[b % N_DISTINCT][0] for b in range(B)])).to(dev)
    depths = torch.from_numpy(np.stack([scenes[b % N_DISTINCT][1] for b in range(B)])).to(dev)
    call = lambda: sel.select_grasp_points_batch(masks, depths)   # noqa: E731
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    whole = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        whole.append(e0.elapsed_time(e1))
    lib.lg_profile_enable(sel._h, 1)
    for _ in range(steps):
        call()
    kern = {}
    for name in STAGES:
        n, ms = C.c_int(0), C.c_double(0.0)
        lib.lg_profile_read(sel._h, name.encode(), C.byref(n), C.byref(ms))
        kern[name + "_ms"] = round(ms.value / max(n.value, 1), 4)
    lib.lg_profile_enable(sel._h, 0)
    print(json.dumps({"B": B, "H": H, "W": W, "top_k": TOP_K, "steps": steps, "lib": os.environ.get("LG_LIB_PATH", "default"),
                      "call_ms_median": round(float(np.median(whole)), 4), "call_ms_min": round(float(np.min(whole)), 4), **kern,
                      "topk_round_us": round(1000.0 * kern["topk_ms"] / TOP_K, 2)}), flush=True)
