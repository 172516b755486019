#!/usr/bin/env python3
"""Deforming geometry: what a refit costs next to a rebuild.

Per scene (Cornell, teapots 100 k, the config-5 1-M-triangle scene), with the scene's own vertices: the first
rdh_scene_refit_geometry after an upload (it derives the refit plan and blocks: wall clock), a steady-state refit and
rdh_scene_update_geometry (hipEvents on the context's stream, warm, best of 5), and the config-3 frame (1080p, depth 8, RDH_PT_AUTO)
after the upload, after a refit and after an update.  One JSON line per scene; --out DIR also writes them to DIR/bvh_refit_rate.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from radish_pt_amd import api, scenes  # noqa: E402


def _events_ms(fn, reps=5):
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
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    row["frame_after_upload_ms"] = _frame_ms(ctx, W, H)
    v = torch.from_numpy(sd.vertices).cuda()
    n = torch.from_numpy(sd.normals).cuda()
    lights = (sd.light_sampler, sd.sum_light_power_inv)
    ctx.synchronize()
    t = time.perf_counter()
    ctx.refit_geometry(v, n, lights)
    ctx.synchronize()
    row["first_refit_wall_ms"] = (time.perf_counter() - t) * 1e3
    row["refit_ms"] = _events_ms(lambda: ctx.refit_geometry(v, n, lights))
    row["frame_after_refit_ms"] = _frame_ms(ctx, W, H)
    now, at_build = ctx.tree_cost()
    row["sah_now"], row["sah_at_build"] = now, at_build
    ctx.update_geometry(v, n, lights)
    ctx.synchronize()
    row["update_geometry_ms"] = _events_ms(lambda: ctx.update_geometry(v, n, lights))
    row["frame_after_update_ms"] = _frame_ms(ctx, W, H)
    row["update_over_refit"] = row["update_geometry_ms"] / row["refit_ms"]
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
        with open(os.path.join(args.out, "bvh_refit_rate.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
