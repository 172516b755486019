#!/usr/bin/env python3
"""What rdh_scene_track_motion costs: rdh_gbuffer_render and the geometry updates with tracking off and on, and the same
calls on another build of the library (the parent commit's tree, --parent-root) alternated with this one in one run.

Per scene (teapots at 1080p, the config-5 1-M-triangle scene at 4K) and build, after 5 warm-up launches, 20 launches per figure,
each reported as median [min, max] in ms:
  gbuffer_static        rdh_gbuffer_render, no update since the last render (tracking off)
  gbuffer_after_update  rdh_gbuffer_render right after a refit (tracking off): the refit restarts the block order, so this is what
                        the tracked figure below compares with
  gbuffer_tracked_static / gbuffer_tracked_after_update   the same two with tracking on; only the last one reads the kept records
  refit / lbvh_update   rdh_scene_refit_geometry / rdh_scene_update_geometry_ex(LBVH) with the scene's own vertices, a render before
                        each (with tracking on it is the first update after a render that keeps the old records), tracking off / on
A build without rdh_scene_track_motion reports the untracked figures only.  The measuring is done by child processes (one per build
and round, `--measure`), because a process can load one build of the library.  --out DIR writes DIR/motion_times.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, LAUNCHES = 5, 20


def _stat(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}


def measure(root, skip_1m):
    sys.path.insert(0, root)
    import torch

    from radish_pt_amd import api, scenes

    def events_ms(fn):
        stream = torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    todo = [("teapots_1080p", lambda: scenes.teapots(), 1920, 1080)]
    if not skip_1m:
        todo.append(("config5_4k", lambda: scenes.teapots(segments=200, bands=156, emissive_grid=(16, 32)), 3840, 2160))
    rows = []
    for name, make, W, H in todo:
        sd = make()
        cam = scenes.teapots_camera(W, H)
        ctx = api.Context(0)
        ctx.upload_scene(sd)
        ctx.set_camera(cam)
        gb = api.GBuffer()
        gb.create(W, H)
        gc = gb.c_struct(cam_fallback=cam)
        v, n = torch.from_numpy(sd.vertices).cuda(), torch.from_numpy(sd.normals).cuda()
        lights = (sd.light_sampler, sd.sum_light_power_inv)
        can_track = hasattr(ctx, "track_motion")
        row = {"scene": name, "triangles": int(sd.num_prims), "width": W, "height": H, "tracking_available": can_track}

        def render():
            ctx.gbuffer_render(gc, 0)
            ctx.synchronize()
            return ctx.last_kernel_ms()

        def refit():
            ctx.refit_geometry(v, n, lights)

        def lbvh():
            ctx.update_geometry(v, n, lights, builder="lbvh")

        def series(fn, before=None):
            ts = []
            for k in range(WARMUP + LAUNCHES):
                if before:
                    before()
                t = fn()
                if k >= WARMUP:
                    ts.append(t)
            return _stat(ts)

        refit()  # the first refit derives the plan and blocks: not part of any figure
        ctx.synchronize()
        for track in ([False, True] if can_track else [False]):
            tag = "_tracked" if track else ""
            if track:
                ctx.track_motion(True)
            row[f"gbuffer{tag}_static"] = series(render)
            row[f"gbuffer{tag}_after_update"] = series(render, before=refit)
            row[f"refit{tag}"] = series(lambda: events_ms(refit), before=render)
            row[f"lbvh_update{tag}"] = series(lambda: events_ms(lbvh), before=render)
            ctx.update_geometry(v, n, lights)  # back to the uploaded tree (the SAH builder gives it bit for bit) and a refit plan,
            refit()                            # so that both passes render the same tree
            ctx.synchronize()
        ctx.close()
        rows.append(row)
    print("MOTION_TIMES " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None, help="a built tree of the parent commit to alternate with this one")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-1m", action="store_true")
    ap.add_argument("--measure", metavar="ROOT", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, args.skip_1m)
    builds = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", HERE)]
    out = []
    for r in range(args.rounds):
        for build, root in builds:
            cmd = [sys.executable, os.path.abspath(__file__), "--measure", root] + (["--skip-1m"] if args.skip_1m else [])
            env = {k: v for k, v in os.environ.items() if k != "RADISH_HIP_LIB"}
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root, timeout=900)
            line = [l for l in p.stdout.splitlines() if l.startswith("MOTION_TIMES ")]
            if p.returncode != 0 or not line:
                sys.exit(f"measuring {build} (round {r}) failed with status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            for row in json.loads(line[0][len("MOTION_TIMES "):]):
                row = {"build": build, "round": r, **row}
                print(json.dumps(row), flush=True)
                out.append(row)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "motion_times.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
