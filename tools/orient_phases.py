#!/usr/bin/env python3
"""Where lg_orient_kernel's time goes: the wall_clock64() stamps a library built with -DLG_ORIENT_PHASES leaves at the phase
boundaries (lg_orient.hip), for the benchmark's masks at one frame and at a batch.
  LG_VARIANT_SRC=lg_orient.hip tools/build_variants.sh "phases:-DLG_ORIENT_PHASES"
  LG_LIB_PATH=leaf-grasping-vision-ml_amd/csrc/variants/liblgrasp_phases.so python tools/orient_phases.py [B=256] [reps=5]
Prints, per batch size, the median over the frames and repetitions of every phase in microseconds (the clock ticks at 100 MHz:
10 ns steps), and the kernel's span from the first frame's start to the last frame's end."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import leafgrasp_amd as L  # noqa: E402
from leafgrasp_amd import _lib  # noqa: E402

PHASES = ["A runs", "B union", "C component", "D row ends", "E hull vertices", "compaction", "F rectangle"]


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    raw = C.CDLL(_lib.LIB_PATH)
    if not hasattr(raw, "lg_debug_orient_phases"):
        sys.exit(f"{_lib.LIB_PATH} was built without -DLG_ORIENT_PHASES")
    raw.lg_debug_orient_phases.restype = C.c_int
    raw.lg_debug_orient_phases.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    H, W = 1080, 1920
    masks_np, depths_np, P, _ = bench.make_frames(B, H, W)
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    sel.set_camera_params(P)
    masks, depths = torch.from_numpy(masks_np).cuda(), torch.from_numpy(depths_np).cuda()
    for nb in sorted({1, B}):
        n = min(nb, 256)
        got = []
        for r in range(reps + 1):
            sel.select_grasp_points_batch(masks[:nb], depths[:nb])
            torch.cuda.synchronize()
            st = np.zeros((n, 8), np.uint64)
            assert raw.lg_debug_orient_phases(st.ctypes.data_as(C.POINTER(C.c_uint64)), n) == 0
            if r:   # (the first call warms up)
                got.append(st.astype(np.int64))
        st = np.stack(got)                              # [reps][frames][8]
        d = np.diff(st, axis=2) * 0.01                  # microseconds
        tot = (st[:, :, 7] - st[:, :, 0]) * 0.01
        span = (st[:, :, 7].max(axis=1) - st[:, :, 0].min(axis=1)) * 0.01
        print(f"{nb} frame(s) of {H} x {W}, {reps} calls: one workgroup's start to end median {np.median(tot):.2f} us "
              f"(min {tot.min():.2f}, max {tot.max():.2f}); first start to last end median {np.median(span):.2f} us")
        for k, name in enumerate(PHASES):
            v = d[:, :, k]
            print(f"  {name:16s} median {np.median(v):7.2f} us  ({100 * np.median(v) / np.median(tot):4.1f} %)  "
                  f"min {v.min():7.2f}  max {v.max():7.2f}")


if __name__ == "__main__":
    main()
