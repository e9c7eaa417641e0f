#!/usr/bin/env python3
"""What the ML-only grasp selection costs: select_grasp_points_ml_batch (lg_select_grasp_ml) at 1080p with the closed-form CNN
weights, B = 1 and 32 by default, for the reference's walk (NTH, target 100) and the score map (GRID, stride 8), against the
route a user had to compose before the entry existed, timed in the same process: dense score_maps, np.where on the host,
gather_patches and cnn_forward per frame, an arg-max in torch.  One JSON line per (B, sampling): the whole call between two
device events on the current stream, the routes alternating, median of `steps` each -- the new call with the library's rule for
the planes, with deferred planes forced (form 1) and with stored planes forced (form 2) -- and the per-launch event times of
the path's kernels from lg_profile_enable (sums per call).
Usage: python tools/ml_select_bench.py [steps] [B ...]"""
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
Bs = [int(a) for a in sys.argv[2:]] or [1, 32]
dev = torch.device("cuda:0")
KERNELS = ("prep", "ml_rows", "ml_table", "ml_list", "final", "gather", "cnn", "ml_pick", "finish", "ml_rows_out")

scenes = []
for s in range(N_DISTINCT):   # the benchmark's scenes: seeds 100.., the largest leaf of each
    labels, depth, P = SI.synthetic_scene(H, W, seed=100 + s)
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    scenes.append((labels == ids[np.argmax(counts)], depth))

sel = L.GraspPointSelector(dev, load_model=False)
sel.set_camera_params(P)
sel.set_cnn_state_dict(SI.cnn_closed_form_params(seed=0))
SAMPLINGS = {"nth100": sel.ml_sampling("nth", target=100), "grid8": sel.ml_sampling("grid", stride=8, max_samples=4096)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def composed(masks, depths, name):
    """the route without the entry: dense planes, the sample list on the host, gather + CNN per frame, arg-max"""
    maps, _, _ = sel.score_maps(masks, depths)
    picks = []
    host = masks.cpu().numpy()
    for b in range(masks.shape[0]):
        ys, xs = np.where(host[b])
        if name == "nth100":
            step = max(1, len(ys) // 100)
            xs, ys = xs[::step], ys[::step]
        else:
            keep = (xs % 8 == 0) & (ys % 8 == 0)
            xs, ys = xs[keep], ys[keep]
        keep = ~((ys < 16) | (ys >= H - 16) | (xs < 16) | (xs >= W - 16))
        pts = np.stack([xs[keep], ys[keep]], 1)
        if not len(pts):
            picks.append(None)
            continue
        patches = sel.gather_patches(masks[b], depths[b], {k: v[b] for k, v in maps.items()}, pts.tolist())
        logits = sel.cnn_forward(patches)
        picks.append(tuple(pts[int(torch.argmax(logits))]))
    return picks


for B in Bs:
    masks = torch.from_numpy(np.stack([scenes[b % N_DISTINCT][0] for b in range(B)])).to(dev)
    depths = torch.from_numpy(np.stack([scenes[b % N_DISTINCT][1] for b in range(B)])).to(dev)
    for name, smp in SAMPLINGS.items():
        def new(form):
            sel.ml_planes(form)
            return sel.select_grasp_points_ml_batch(masks, depths, sampling=smp)
        routes = {"rule": lambda: new(0), "deferred": lambda: new(1), "stored": lambda: new(2),
                  "composed": lambda: composed(masks, depths, name)}
        for fn in routes.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        order = list(routes)
        for i in range(steps):   # alternate, rotating which route goes first
            for k in order[i % len(order):] + order[:i % len(order)]:
                times[k].append(timed(routes[k]))
        new(0)
        rule_form = sel.ml_planes(0)
        _, rows, counts = sel.select_grasp_points_ml_batch(masks, depths, sampling=smp, return_samples=True)
        scored = int(sum(rows["scored"][b, :max(int(counts[b]), 0)].sum() for b in range(B)))
        kern = {}
        for form, tag in ((0, "rule"), (1, "deferred"), (2, "stored")):   # per-launch event times, summed per call
            new(form)
            lib.lg_profile_enable(sel._h, 1)
            for _ in range(steps):
                new(form)
            kern[tag] = {}
            for kname in KERNELS if form == 0 else ("final", "gather"):
                n, ms = C.c_int(0), C.c_double(0.0)
                lib.lg_profile_read(sel._h, kname.encode(), C.byref(n), C.byref(ms))
                kern[tag][kname + "_ms"] = round(ms.value / steps, 4)
            lib.lg_profile_enable(sel._h, 0)
        sel.ml_planes(0)
        med = {k + "_ms_median": round(float(np.median(v)), 4) for k, v in times.items()}
        mn = {k + "_ms_min": round(float(np.min(v)), 4) for k, v in times.items()}
        print(json.dumps({"B": B, "H": H, "W": W, "sampling": name, "steps": steps, "patches": scored, "rule_form": rule_form, **med, **mn,
                          "kernels_per_call": kern}), flush=True)
