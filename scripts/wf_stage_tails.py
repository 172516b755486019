#!/usr/bin/env python3
"""Diagnostic: where each wavefront trace stage's queue runs dry and how long the stage goes on after that.

Needs a -DRD_WF_STAMPS build of the library via RADISH_HIP_LIB (radish_pt_amd/_build.py, build_variant): every wave of k_wf_trace
stamps the wall clock (100 MHz) when it enters, when it first finds the stage's queue exhausted, when it leaves and when it has left
the list loop, and says how many reserved items it held when the shared head was dry (kernels_wave.h, kWfStampKinds).  Renders the
headline workload (teapots, 1920x1080, 8 bounces, wavefront + material sort, one pipeline) and prints, per stage, in us from the
launch's start (the stage's earliest entry stamp), the median over the timed frames of
    dry    the first wave finding the queue dry (waves whose static first packet already lies beyond the stage's items are left
           out of this and counted under "idle": they never had work)
    tail   from then to the last wave leaving
    p50    the median wave's exit
    span   the last wave's exit
    p50>   from the median wave's exit to the last one's: what imbalance between waves costs
and a second table that says where the last waves come from.  A workgroup has LIST DUTY when its ticket is below the stage's list
length (the stamps carry it): its four waves trace a literal-class ray together before anything else.  Per stage
    L            workgroups with list duty
    list us      of those, the time from entry to leaving the list loop: median, 90th percentile, max
    exit duty    the exit (us from the launch's start) of the workgroups with list duty: median, 90th percentile, max
    exit others  the same of the others that had work
    last 100 us  waves that leave in the stage's last 100 us: how many, how many of them belong to duty workgroups, how many still
                 held reserved items they had not started when the shared head was dry (their own and their workgroup's)
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
rows2 = []  # [frame][stage] = (L, list p50 p90 max, duty exit p50 p90 max, others' exit p50 p90 max, last: waves, of duty, holding)


def pct(x):
    return (np.median(x), np.percentile(x, 90), x.max()) if x.size else (0.0, 0.0, 0.0)



for f in range(frames):
    ctx.path_trace(d, i, 2 + f, 2 + f, depth, flags)
    ctx.synchronize()
    ms = ctx.last_kernel_ms()
    st = ctx.debug_wf_stamps().astype(np.float64) / 100.0  # us
    raw = ctx.debug_wf_stamps()
    per, per2 = [], []
    for k in range(st.shape[0]):
        ran = st[k, :, 0] > 0
        entry, dry, out = st[k, ran, 0], st[k, ran, 1], st[k, ran, 2]
        t0 = entry.min()
        worked = dry - entry > 2.0
        first_dry = (dry[worked].min() if worked.any() else dry.min()) - t0
        per.append((first_dry, out.max() - t0 - first_dry, np.median(out) - t0, out.max() - t0, int((~worked).sum()), int(ran.sum())))
        # by workgroup (four consecutive logical waves); workgroups of which not every wave ran are left out
        g = st[k].reshape(-1, 4, st.shape[2])
        g = g[(g[:, :, 0] > 0).all(axis=1)]  # (their tickets: `tickets` below)
        n_lit = int(raw[k, :, 5].max()) - 1
        tickets = np.nonzero((st[k].reshape(-1, 4, st.shape[2])[:, :, 0] > 0).all(axis=1))[0]
        wg_duty = tickets < n_lit
        wg_exit = g[:, :, 2].max(axis=1) - t0
        wg_list = (g[:, :, 3] - g[:, :, 0]).max(axis=1)
        wg_worked = ((g[:, :, 1] - g[:, :, 0]) > 2.0).any(axis=1)
        last = out >= out.max() - 100.0
        wave_duty = (np.nonzero(ran)[0] // 4) < n_lit
        held = raw[k, ran, 4] > 1
        per2.append((int(wg_duty.sum()),) + pct(wg_list[wg_duty]) + pct(wg_exit[wg_duty]) + pct(wg_exit[~wg_duty & wg_worked])
                    + (int(last.sum()), int((last & wave_duty).sum()), int((last & held).sum())))
    rows.append((ms, per))
    rows2.append(per2)
print(f"{os.path.basename(os.environ.get('RADISH_HIP_LIB', 'default library'))}: {scene} {W}x{H}, depth {depth}, {frames} frames; "
      f"frame ms (stamped build) {' '.join(f'{ms:.3f}' for ms, _ in rows)}")
print("stage   waves  idle      dry     tail      p50     span     p50>   (us, median of the frames)")
a = np.array([per for _, per in rows])  # [frame][stage][6]
med = np.median(a, axis=0)
for k in range(med.shape[0]):
    print(f"{k:5d} {int(med[k, 5]):7d} {int(med[k, 4]):5d} {med[k, 0]:8.1f} {med[k, 1]:8.1f} {med[k, 2]:8.1f} {med[k, 3]:8.1f} {med[k, 3] - med[k, 2]:8.1f}")
print(f"  sum {'':13s} {med[:, 0].sum():8.1f} {med[:, 1].sum():8.1f} {med[:, 2].sum():8.1f} {med[:, 3].sum():8.1f} {(med[:, 3] - med[:, 2]).sum():8.1f}")
print(f"stages 1..{med.shape[0] - 1}: dry {med[1:, 0].sum():.1f}  tail {med[1:, 1].sum():.1f}  span {med[1:, 3].sum():.1f}  "
      f"median-to-last {(med[1:, 3] - med[1:, 2]).sum():.1f}")
m2 = np.median(np.array(rows2, dtype=np.float64), axis=0)  # [stage][13]
print("where the last waves come from (us, median of the frames; p50 / p90 / max)")
print("stage     L          list us of duty workgroups         exit of duty workgroups              exit of the others   last 100 us: waves / of duty / holding")
for k in range(m2.shape[0]):
    r = m2[k]
    print(f"{k:5d} {int(r[0]):5d}   {r[1]:8.1f} {r[2]:8.1f} {r[3]:8.1f}   {r[4]:8.1f} {r[5]:8.1f} {r[6]:8.1f}   {r[7]:8.1f} {r[8]:8.1f} {r[9]:8.1f}   "
      f"{int(r[10]):6d} {int(r[11]):6d} {int(r[12]):6d}")
ctx.close()
