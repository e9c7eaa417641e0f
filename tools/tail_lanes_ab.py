#!/usr/bin/env python3
"""A/B of the tail lanes of lg_select_grasp ("Tail in lanes") on one handle: bench.py's frames, its timed
loop, the lanes forced through lg_debug_tail_lanes.

    python tools/tail_lanes_ab.py [--batches 32,64,128,256] [--lanes 1,2,3,4] [--rounds 3] [--steps 20] [--warmup 5]

Every (batch, lanes) pair is timed once per round, the settings alternating inside a round, so that a drift of the machine
shows as a difference between rounds and not between settings.  Prints one JSON line per reading and a closing summary line:
per batch and setting every reading in ms per step, and `wins`: the settings whose every reading beats every lanes-1 reading.
profiles/NOTES_tail_lanes.md says how LG_TAIL_LANES_AUTO and LG_TAIL_LANES_MIN_B follow from it."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (make_frames: the benchmark's scenes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,64,128,256")
    ap.add_argument("--lanes", default="1,2,3,4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    batches = [int(x) for x in args.batches.split(",")]
    lanes = [int(x) for x in args.lanes.split(",")]
    H, W = args.height, args.width
    masks_np, depths_np, P, _ = bench.make_frames(max(batches), H, W, workers=max(1, min(8, bench._cpu_share())))

    import torch

    import leafgrasp_amd as L
    import synthetic_inputs as SI

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    masks, depths = torch.from_numpy(masks_np).to(dev), torch.from_numpy(depths_np).to(dev)
    sel = L.GraspPointSelector(dev, load_model=False)
    sel.set_camera_params(P)
    sel.set_cnn_state_dict(SI.cnn_closed_form_params(seed=0))
    stream = torch.cuda.Stream(dev)
    readings = {B: {n: [] for n in lanes} for B in batches}
    with torch.cuda.stream(stream):
        for B in sorted(batches, reverse=True):   # (the largest first: the workspace is sized once)
            m, d = masks[:B], depths[:B]
            for rnd in range(args.rounds):
                for n in lanes:
                    sel.tail_lanes(n)
                    for _ in range(args.warmup):
                        sel.select_grasp_points_batch(m, d)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        sel.select_grasp_points_batch(m, d)
                    torch.cuda.synchronize(dev)
                    ms = 1e3 * (time.perf_counter() - t0) / args.steps
                    ran = sel.tail_lanes()
                    readings[B][n].append(round(ms, 4))
                    print(json.dumps({"B": B, "round": rnd, "lanes": n, "ran_lanes": ran, "ms_per_step": round(ms, 4)}), flush=True)
    summary = {}
    for B in batches:
        base = readings[B].get(1, [])
        summary[str(B)] = {"ms_per_step": {str(n): readings[B][n] for n in lanes},
                           "wins": [n for n in lanes if n != 1 and base and max(readings[B][n]) < min(base)]}
    print(json.dumps({"summary": summary, "height": H, "width": W, "steps": args.steps, "rounds": args.rounds}), flush=True)


if __name__ == "__main__":
    main()
