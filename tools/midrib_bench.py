#!/usr/bin/env python3
"""Device time of lg_detect_midrib (GraspPointSelector.detect_midrib_batch) at 1080p, B = 1, 32, 256 by default: one JSON
line per B with the whole call between two device events (median of `steps` calls) and the per-kernel event times of the
call's stages (lg_profile_enable).  hist_hbm_frac = H * W * (1 + C) bytes per frame / histogram time / HBM peak.
Usage: python tools/midrib_bench.py [steps] [B ...]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import leafgrasp_amd as L  # noqa: E402
from leafgrasp_amd._lib import lib  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s
H, W, CH = 1080, 1920, 3
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
Bs = [int(a) for a in sys.argv[2:]] or [1, 32, 256]
dev = torch.device("cuda:0")


def scenes(B, seed=0):
    """Elliptical leaves (about 6 per cent of the frame) with a brighter ridge on noise, made on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    p = torch.rand((B, 5), generator=g, device=dev)
    cx, cy = (0.3 + 0.4 * p[:, 0]) * W, (0.3 + 0.4 * p[:, 1]) * H
    th, a = p[:, 2] * np.pi, (0.2 + 0.1 * p[:, 3]) * H
    b = a * (0.3 + 0.2 * p[:, 4])
    dx, dy = xx[None] - cx[:, None, None], yy[None] - cy[:, None, None]
    u = dx * torch.cos(th)[:, None, None] + dy * torch.sin(th)[:, None, None]
    v = -dx * torch.sin(th)[:, None, None] + dy * torch.cos(th)[:, None, None]
    inside = (u / a[:, None, None]) ** 2 + (v / b[:, None, None]) ** 2 <= 1
    img = torch.randint(0, 70, (B, H, W, CH), generator=g, device=dev, dtype=torch.int32)
    leaf = torch.randint(20, 70, (B, H, W, CH), generator=g, device=dev, dtype=torch.int32)
    leaf[..., 1] += 90
    leaf += ((v.abs() < 0.1 * b[:, None, None]).to(torch.int32) * 60)[..., None]
    img = torch.where(inside[..., None], leaf, img).clamp(0, 255).to(torch.uint8).contiguous()
    return inside.to(torch.uint8).contiguous(), img


sel = L.GraspPointSelector(dev, load_model=False)
for B in Bs:
    masks, imgs = scenes(B)
    for _ in range(3):
        sel.detect_midrib_batch(masks, imgs)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = sel.detect_midrib_batch(masks, imgs)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    lib.lg_profile_enable(sel._h, 1)
    for _ in range(steps):
        sel.detect_midrib_batch(masks, imgs)
    kern = {}
    for name in ("midrib_hist", "midrib_lut", "midrib_orient", "midrib_walk"):
        n, ms = C.c_int(0), C.c_double(0.0)
        lib.lg_profile_read(sel._h, name.encode(), C.byref(n), C.byref(ms))
        kern[name + "_ms"] = round(ms.value / max(n.value, 1), 4)
    lib.lg_profile_enable(sel._h, 0)
    hist_s = kern["midrib_hist_ms"] * 1e-3
    out = {"B": B, "H": H, "W": W, "C": CH, "steps": steps, "call_ms_median": round(float(np.median(times)), 4),
           "call_ms_min": round(float(np.min(times)), 4), **kern,
           "hist_hbm_frac": round(B * H * W * (1 + CH) / hist_s / HBM_PEAK, 3) if hist_s > 0 else None,
           "found": sum(r is not None for r in res)}
    print(json.dumps(out), flush=True)
