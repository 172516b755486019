#!/usr/bin/env python3
"""The LBVH rebuild next to the SAH rebuild and the refit.

Per scene (Cornell, teapots 100 k, the config-5 1-M-triangle scene), with the scene's own vertices: build_bvh_device(lbvh),
update_geometry(lbvh), update_geometry(sah) and a steady-state refit (hipEvents on the context's stream, after a warm-up call, best
of 5); tree_cost of the SAH and the LBVH tree; the config-3 frame (1080p, depth 8, RDH_PT_AUTO) after an SAH update and after an
LBVH update, with the nodeVisits / triTests counters of a separate counted frame.  One JSON line per scene; --out DIR also writes
them to DIR/bvh_lbvh_rate.json.  --only-lbvh-update N runs N LBVH updates of the 1-M scene and nothing else (for a kernel trace)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from radish_pt_amd import api, scenes  # noqa: E402


def _events_ms(ctx, fn, reps=5):
    fn()  # warm-up
    ctx.synchronize()
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


def _frame(ctx, W, H, reps=3):
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    ts = []
    for _ in range(reps):
        ctx.path_trace(d, i, 0, 1, 8, api.RDH_PT_AUTO)
        ctx.synchronize()
        ts.append(ctx.last_kernel_ms())
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, 1, 8, api.RDH_PT_AUTO | api.RDH_PT_COUNT)
    ctx.synchronize()
    c = ctx.counters()
    return min(ts), {k: c[k] for k in ("nodeVisits", "triTests") if k in c}


def run(name, sd, cam, W, H):
    ctx = api.Context(0)
    row = {"scene": name, "triangles": int(sd.num_prims)}
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    v = torch.from_numpy(sd.vertices).cuda()
    n = torch.from_numpy(sd.normals).cuda()
    lights = (sd.light_sampler, sd.sum_light_power_inv)
    row["build_bvh_device_lbvh_ms"] = _events_ms(ctx, lambda: ctx.build_bvh_device(v, builder="lbvh"))
    row["update_geometry_sah_ms"] = _events_ms(ctx, lambda: ctx.update_geometry(v, n, lights))
    row["sah_tree_cost"] = ctx.tree_cost()[0]
    row["frame_after_sah_update_ms"], row["counters_after_sah_update"] = _frame(ctx, W, H)
    row["update_geometry_lbvh_ms"] = _events_ms(ctx, lambda: ctx.update_geometry(v, n, lights, builder="lbvh"))
    row["lbvh_tree_cost"] = ctx.tree_cost()[0]
    row["frame_after_lbvh_update_ms"], row["counters_after_lbvh_update"] = _frame(ctx, W, H)
    ctx.refit_geometry(v, n, lights)  # derives the plan (blocking)
    row["refit_ms"] = _events_ms(ctx, lambda: ctx.refit_geometry(v, n, lights))
    row["sah_update_over_lbvh_update"] = row["update_geometry_sah_ms"] / row["update_geometry_lbvh_ms"]
    row["lbvh_cost_over_sah_cost"] = row["lbvh_tree_cost"] / row["sah_tree_cost"]
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-lbvh-update", type=int, default=0)
    args = ap.parse_args()
    W, H = 1920, 1080
    big = ("config5_1m", lambda: scenes.teapots(segments=200, bands=156, emissive_grid=(16, 32)), scenes.teapots_camera(W, H))
    if args.only_lbvh_update:
        sd = big[1]()
        ctx = api.Context(0)
        ctx.upload_scene(sd)
        v, n = torch.from_numpy(sd.vertices).cuda(), torch.from_numpy(sd.normals).cuda()
        for _ in range(args.only_lbvh_update):
            ctx.update_geometry(v, n, (sd.light_sampler, sd.sum_light_power_inv), builder="lbvh")
        ctx.synchronize()
        ctx.close()
        return
    todo = [("cornell", scenes.cornell, scenes.cornell_camera(W, H)), ("teapots", scenes.teapots, scenes.teapots_camera(W, H)), big]
    rows = []
    for name, make, cam in todo:
        r = run(name, make(), cam, W, H)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bvh_lbvh_rate.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
