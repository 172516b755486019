#!/usr/bin/env python3
"""Diagnostic: where each wavefront trace stage's queue runs dry and how long the stage goes on after that.

Needs a -DRD_WF_STAMPS build of the library via RADISH_HIP_LIB (radish_pt_amd/_build.py, build_variant): every wave of k_wf_trace
stamps the wall clock (100 MHz) when it enters, when it first finds the stage's queue exhausted, and when it leaves.  Renders the
headline workload (teapots, 1920x1080, 8 bounces, wavefront + material sort, one pipeline) and prints, per stage, in us from the
launch's start (the stage's earliest entry stamp), the median over the timed frames of
    dry    the first wave finding the queue dry (waves whose static first packet already lies beyond the stage's items are left
           out of this and counted under "idle": they never had work)
    tail   from then to the last wave leaving
    p50    the median wave's exit
    span   the last wave's exit
Usage: RADISH_HIP_LIB=<stamped build> python scripts/wf_stage_tails.py [frames=5] [scene=teapots] [depth=8]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radish_pt_amd import api, scenes  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scene = sys.argv[2] if len(sys.argv) > 2 else "teapots"
depth = int(sys.argv[3]) if len(sys.argv) > 3 else 8
W, H = 1920, 1080
sd = scenes.cornell() if scene == "cornell" else scenes.teapots()
cam = scenes.cornell_camera(W, H) if scene == "cornell" else scenes.teapots_camera(W, H)
flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES
ctx = api.Context(0)
ctx.upload_scene(sd)
ctx.set_camera(cam)
d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
for it in range(2):  # warm-up
    ctx.path_trace(d, i, it, it, depth, flags)
ctx.synchronize()
rows = []  # [frame][stage] = (dry, tail, p50, span, idle waves, frame ms)
for f in range(frames):
    ctx.path_trace(d, i, 2 + f, 2 + f, depth, flags)
    ctx.synchronize()
    ms = ctx.last_kernel_ms()
    st = ctx.debug_wf_stamps().astype(np.float64) / 100.0  # us
    per = []
    for k in range(st.shape[0]):
        ran = st[k, :, 0] > 0
        entry, dry, out = st[k, ran, 0], st[k, ran, 1], st[k, ran, 2]
        t0 = entry.min()
        worked = dry - entry > 2.0
        first_dry = (dry[worked].min() if worked.any() else dry.min()) - t0
        per.append((first_dry, out.max() - t0 - first_dry, np.median(out) - t0, out.max() - t0, int((~worked).sum()), int(ran.sum())))
    rows.append((ms, per))
print(f"{os.path.basename(os.environ.get('RADISH_HIP_LIB', 'default library'))}: {scene} {W}x{H}, depth {depth}, {frames} frames; "
      f"frame ms (stamped build) {' '.join(f'{ms:.3f}' for ms, _ in rows)}")
print("stage   waves  idle      dry     tail      p50     span   (us, median of the frames)")
a = np.array([per for _, per in rows])  # [frame][stage][6]
med = np.median(a, axis=0)
for k in range(med.shape[0]):
    print(f"{k:5d} {int(med[k, 5]):7d} {int(med[k, 4]):5d} {med[k, 0]:8.1f} {med[k, 1]:8.1f} {med[k, 2]:8.1f} {med[k, 3]:8.1f}")
print(f"  sum {'':13s} {med[:, 0].sum():8.1f} {med[:, 1].sum():8.1f} {med[:, 2].sum():8.1f} {med[:, 3].sum():8.1f}")
print(f"stages 1..{med.shape[0] - 1}: dry {med[1:, 0].sum():.1f}  tail {med[1:, 1].sum():.1f}  span {med[1:, 3].sum():.1f}")
ctx.close()
