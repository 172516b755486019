#!/usr/bin/env python3
"""Records per stage of a wavefront frame: rayCount[k] (extension rays of trace(k) = records of shade(k)) and shadowCount[k] (shadow
rays shade(k) emits, traced by trace(k + 1)), untimed, from the RDH_PT_COUNT counters of frames of depth 0 .. D: a frame of depth d
runs stages 0 .. d, so stage d's rays are the difference between two depths' counts.
usage: wf_stage_records.py <scene> <mode> <W> <H> <depth>      prints one line per stage: k rays shadow"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from radish_pt_amd import api
import bench

scene, mode, W, H, D = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
ctx = api.Context(0)
ctx.upload_scene(bench.make_scene(scene))
ctx.set_camera(bench.make_camera(scene, W, H))
d = torch.zeros(W * H, 3, device="cuda"); i = torch.zeros(W * H, 3, device="cuda")
flags = bench.mode_flags(api, mode) | api.RDH_PT_COUNT
closest, anyr = [], []
for depth in range(D + 1):
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, 0, depth, flags)
    ctx.synchronize()
    c = ctx.counters()
    closest.append(c["closestRays"]); anyr.append(c["anyRays"])
print(f"# {scene} {mode} {W}x{H}, looper 0: k rayCount[k] shadowCount[k]")
for k in range(D + 1):
    rays = closest[k] - (closest[k - 1] if k else 0)
    shadow = (anyr[k + 1] - anyr[k]) if k < D else 0  # shade(D) emits none: the depth bound
    print(k, rays, shadow)
ctx.close()
