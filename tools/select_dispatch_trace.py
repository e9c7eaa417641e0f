#!/usr/bin/env python3
"""Kernel dispatches per hardware queue of one call of every form the selection entries take, for comparing two builds of the
library (LG_LIB_PATH selects the other one) after a change of the host orchestration in csrc/lg_select.hip.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/select_dispatch_trace.py run
    python tools/select_dispatch_trace.py table OUT > a.json        # {form: [[kernel names of queue 0 in dispatch order], ...]}
    python tools/select_dispatch_trace.py compare a.json b.json     # a markdown table: kernels per queue, same or not

`run` makes one call per form, 192 x 256 frames of the synthetic scenes, and launches torch's spin kernel between two forms:
`table` cuts the trace at those.  Queues are numbered per form in the order of their first dispatch."""
import csv
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FORMS = ("select B=4, automatic", "select B=4, 2 lanes", "select B=4, 3 lanes asked (2 + 2 frames: two)", "select B=5, 3 lanes",
         "candidates B=4", "labels B=4, label_aware=1", "select B=4, planes taken back", "select B=5, LG_SUBBATCH=2", "select_ml B=4",
         "select_collect B=4", "score_maps B=4")
H, W = 192, 256


def run():
    import numpy as np
    import torch

    import leafgrasp_amd as L
    from leafgrasp_amd.collecting_selector import CollectingGraspPointSelector
    import synthetic_inputs as O   # (seeded scenes and the closed-form CNN weights)

    dev = torch.device("cuda:0")
    scenes = [O.synthetic_scene(H, W, seed) for seed in (3, 4, 12, 6, 9)]
    labels = torch.from_numpy(np.stack([s[0] for s in scenes]).astype(np.int16)).to(dev)
    depth = torch.from_numpy(np.stack([s[1] for s in scenes])).to(dev)
    mask = (labels == 1).to(torch.uint8)
    weights = O.cnn_closed_form_params(seed=0)

    def selector(cls=L.GraspPointSelector, **env):
        os.environ.update(env)
        sel = cls(dev) if cls is CollectingGraspPointSelector else cls(dev, load_model=False)
        for k in env:
            del os.environ[k]
        sel.set_camera_params(scenes[0][2])
        if cls is L.GraspPointSelector:
            sel.set_cnn_state_dict(weights)
        return sel

    sel, piped, col = selector(), selector(LG_SUBBATCH="2"), selector(CollectingGraspPointSelector)

    def lanes(n, B=4):
        sel.tail_lanes(n)
        sel.select_grasp_points_batch(mask[:B], depth[:B])

    calls = (lambda: lanes(0), lambda: lanes(2), lambda: lanes(3), lambda: lanes(3, 5),
             lambda: sel.select_grasp_candidates_batch(mask[:4], depth[:4]),
             lambda: sel.select_grasp_points_for_leaves(labels[:4].contiguous(), [1] * 4, depth[:4], label_aware=True),
             lambda: sel.select_grasp_points_batch(mask[:4], depth[:4], return_maps=True),
             lambda: piped.select_grasp_points_batch(mask, depth),
             lambda: sel.select_grasp_points_ml_batch(mask[:4], depth[:4]),
             lambda: col.select_grasp_points_batch(mask[:4], depth[:4]),
             lambda: sel.score_maps(mask[:4], depth[:4]))
    assert len(calls) == len(FORMS)
    for name, call in zip(FORMS, calls):
        torch.cuda.synchronize()
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        print(name, "ran; tail lanes", sel.tail_lanes(), flush=True)


def table(out_dir):
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*_kernel_trace.csv"), recursive=True))
    rows = list(csv.DictReader(open(files[-1])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    forms = []
    for r in rows:
        name = r["Kernel_Name"]
        if "spin_kernel" in name:
            forms.append({})
        elif forms:
            forms[-1].setdefault(r["Queue_Id"], []).append(name)
    assert len(forms) == len(FORMS), (len(forms), "segments in the trace", sorted({r["Kernel_Name"][:60] for r in rows}))
    json.dump({n: list(q.values()) for n, q in zip(FORMS, forms)}, sys.stdout, indent=1)


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    print("| form | kernels per queue, first build | second build | names in order per queue |\n|---|---|---|---|")
    same = True
    for n in FORMS:
        same = same and a[n] == b[n]
        print(f"| {n} | {' + '.join(str(len(q)) for q in a[n])} | {' + '.join(str(len(q)) for q in b[n])} |"
              f" {'the same' if a[n] == b[n] else 'DIFFER'} |")
    short = lambda k: k[k.find("lg_") + 3:].split("(")[0].split("<")[0].replace("_kernel", "") if "lg_" in k else k.split("(")[0][-24:]
    for n in FORMS:
        print(f"\n{n}:")
        for i, q in enumerate(a[n]):
            print(f"- queue {i}: {' '.join(short(k) for k in q)}")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    {"run": run, "table": table, "compare": compare}[sys.argv[1]](*sys.argv[2:])
