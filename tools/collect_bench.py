#!/usr/bin/env python3
"""What the collecting selector costs: CollectingGraspPointSelector.select_grasp_points_batch (lg_select_grasp_collect) on one
1080 x 1920 frame, against GraspPointSelector.select_grasp_points_batch without a model (lg_select_grasp) -- the only yardstick
there is: no earlier route produced the variant's planes.  The two calls alternate in one process, so both see the same clock
state; each is timed between two device events on the current stream; medians of `steps`.  Also the collecting call with
every plane taken back (what select_grasp_point does when a collector is attached), and the per-launch event times of the
path's kernels from lg_profile_enable.  One JSON line.
Usage: python tools/collect_bench.py [steps]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import leafgrasp_amd as L  # noqa: E402
import synthetic_inputs as SI  # noqa: E402
from leafgrasp_amd._lib import lib  # noqa: E402

H, W = 1080, 1920
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")
KERNELS = ("prep", "col_erode", "bbox", "dt_fwd", "dt_bwd", "dt_search", "orient", "stem", "final", "col_tip", "col_fuse", "col_pick",
           "finish")

_, depth, P = SI.synthetic_scene(H, W, seed=100)
yy, xx = np.mgrid[0:H, 0:W]
ca, sa = np.cos(0.3), np.sin(0.3)
u, v = (xx - 900) * ca + (yy - 500) * sa, -(xx - 900) * sa + (yy - 500) * ca
mask = torch.from_numpy(((u / 420.0) ** 2 + (v / 280.0) ** 2 <= 1.0)[None]).to(dev)   # a leaf that keeps a safe zone
depth = torch.from_numpy(depth[None]).to(dev)

sel = L.GraspPointSelector(dev, load_model=False)
col = L.CollectingGraspPointSelector(dev)
sel.set_camera_params(P)
col.set_camera_params(P)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


routes = {"select_grasp": lambda: sel.select_grasp_points_batch(mask, depth),
          "collect": lambda: col.select_grasp_points_batch(mask, depth),
          "collect_planes_back": lambda: col.select_grasp_points_batch(mask, depth, return_maps=True)}
times = {k: [] for k in routes}
for i in range(5 + steps):
    for k, fn in routes.items():
        t = timed(fn)
        if i >= 5:
            times[k].append(t)
row = col.last_results[0]
out = {"H": H, "W": W, "steps": steps, "mask_px": int(mask.sum()), "found": int(row.found), "n_candidates": int(row.n_candidates),
       "ms_median": {k: round(statistics.median(v), 4) for k, v in times.items()},
       "ms_min": {k: round(min(v), 4) for k, v in times.items()}, "tip_aware_1": "not built (LG_ERR_UNSUPPORTED)"}
lib.lg_profile_enable(col._h, 1)
for _ in range(steps):
    col.select_grasp_points_batch(mask, depth)
per = {}
for name in KERNELS:
    n, ms = C.c_int(), C.c_double()
    lib.lg_profile_read(col._h, name.encode(), C.byref(n), C.byref(ms))
    if n.value:
        per[name] = {"launches_per_call": n.value / steps, "ms_per_call": round(ms.value / steps, 4)}
lib.lg_profile_enable(col._h, 0)
out["kernels"] = per
print(json.dumps(out))
