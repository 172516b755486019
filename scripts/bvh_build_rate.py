#!/usr/bin/env python3
"""Moving geometry: what a changed scene costs before its next frame.

Per scene (Cornell, teapots 100 k, the config-5 1-M-triangle scene): the host builder rdh_build_bvh and the full
rdh_scene_upload, the device builder rdh_build_bvh_device and rdh_scene_update_geometry (hipEvents on the context's stream,
warm, best of 5), and the config-3 frame (1080p, depth 8, RDH_PT_AUTO) right after an update next to the same frame after an
upload.  One JSON line per scene; --out DIR also writes them to DIR/bvh_build_rate.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from radish_pt_amd import api, hostlib, scenes  # noqa: E402


def _events_ms(ctx, fn, reps=5):
    stream = torch.cuda.current_stream()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def _wall_ms(fn, reps=3):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t) * 1e3)
    return best


def _frame_ms(ctx, W, H, reps=3):
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    ts = []
    for _ in range(reps):
        ctx.path_trace(d, i, 0, 1, 8, api.RDH_PT_AUTO)
        ctx.synchronize()
        ts.append(ctx.last_kernel_ms())
    return min(ts)


def run(name, sd, cam, W, H):
    ctx = api.Context(0)
    row = {"scene": name, "triangles": int(sd.num_prims)}
    row["host_build_ms"] = _wall_ms(lambda: hostlib.build_bvh(sd.vertices))
    row["upload_ms"] = _wall_ms(lambda: ctx.upload_scene(sd))
    ctx.set_camera(cam)
    row["frame_after_upload_ms"] = _frame_ms(ctx, W, H)
    v = torch.from_numpy(sd.vertices).cuda()
    n = torch.from_numpy(sd.normals).cuda()
    ctx.build_bvh_device(v)  # warm (workspace allocation)
    row["device_build_ms"] = _events_ms(ctx, lambda: ctx.build_bvh_device(v))
    lights = (sd.light_sampler, sd.sum_light_power_inv)
    ctx.update_geometry(v, n, lights)
    ctx.synchronize()
    row["update_geometry_ms"] = _events_ms(ctx, lambda: ctx.update_geometry(v, n, lights))
    row["frame_after_update_ms"] = _frame_ms(ctx, W, H)
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-1m", action="store_true")
    args = ap.parse_args()
    W, H = 1920, 1080
    todo = [("cornell", scenes.cornell(), scenes.cornell_camera(W, H)),
            ("teapots", scenes.teapots(), scenes.teapots_camera(W, H))]
    if not args.skip_1m:
        todo.append(("config5_1m", scenes.teapots(segments=200, bands=156, emissive_grid=(16, 32)), scenes.teapots_camera(W, H)))
    rows = []
    for name, sd, cam in todo:
        r = run(name, sd, cam, W, H)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bvh_build_rate.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
