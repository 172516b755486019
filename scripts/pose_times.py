#!/usr/bin/env python3
"""What posing objects on the device costs: rdh_scene_pose_objects against what a caller had to do before it.

Per scene (teapots, 100 364 triangles; the config-5 scene, 999 436 triangles): an object table of the 16 stand-ins over their
ranges of the uploaded soup, rest pose = the uploaded vertices.  Each figure is taken with an event pair on the context's stream
around the call, after 5 warm-up calls, over 20 calls, and reported as median [min, max] in ms; the three figures are taken in
turn, `--rounds` times over (the alternation of scripts/motion_times.py, here between calls of one build):
  pose_all     pose_objects(all 16, tree="refit"): staging, k_pose_objects, k_geom_update, k_refit
  pose_one     pose_objects(one object, tree="refit"): the refit still covers the whole scene
  torch_refit  the same arrays by a torch expression on the device (one batched matrix product per array over the 16 ranges, the
               normals normalised, the 16 matrices uploaded per call) followed by refit_geometry: what a caller does today
Every call moves the objects to a new pose (a small rotation about y and a translation that change with the call).
--out DIR writes DIR/pose_times.json."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
WARMUP, LAUNCHES = 5, 20


def _stat(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-1m", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from radish_pt_amd import api, hostlib, scenes

    def events_ms(fn):
        stream = torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    todo = [("teapots", 64, 49, None)]
    if not args.skip_1m:
        todo.append(("config5", 200, 156, (16, 32)))
    out = []
    for name, segments, bands, emissive in todo:
        sd = scenes.teapots(segments=segments, bands=bands, emissive_grid=emissive)
        per = segments * bands * 2
        first = 12  # the room's 10 triangles and the ceiling light's 2 come first (scenes.teapots)
        table = np.zeros(16, api.OBJECT_RANGE_DTYPE)
        table["firstPrim"] = first + per * np.arange(16)
        table["numPrims"] = per
        table["restFirstPrim"] = table["firstPrim"]
        assert first + 16 * per <= sd.num_prims
        ctx = api.Context(0)
        ctx.upload_scene(sd)
        ctx.set_objects(objects=table, rest_vertices=sd.vertices, rest_normals=sd.normals)
        rest_v = torch.from_numpy(sd.vertices).cuda()
        rest_n = torch.from_numpy(sd.normals).cuda()
        world_v, world_n = rest_v.clone(), rest_n.clone()
        lo, hi = 3 * first, 3 * (first + 16 * per)
        call = [0]

        def xforms(count):
            call[0] += 1
            k = call[0]
            return np.stack([hostlib.object_transform((0.001 * (k % 7), 0.0, 0.0005 * j), (0.0, 0.05 * ((k + j) % 11), 0.0), (1.0, 1.0, 1.0))
                             for j in range(count)])

        def pose_all():
            xf = xforms(16)
            return events_ms(lambda: ctx.pose_objects(np.arange(16), xforms=xf, tree="refit"))

        def pose_one():
            xf = xforms(1)
            return events_ms(lambda: ctx.pose_objects([call[0] % 16], xforms=xf, tree="refit"))

        def torch_refit():
            xf = xforms(16)

            def run():
                m = torch.from_numpy(xf).cuda().view(16, 2, 4, 4)  # [object][X | inverse][col][row]
                X, Xi = m[:, 0], m[:, 1]
                # w = p . X[:3, :] + X[3, :]  (row vector times the column-major matrix);  nn[r] = sum_c Xi[r][c] n[c]
                world_v[lo:hi].view(16, 3 * per, 3).copy_(torch.baddbmm(X[:, 3:4, :3], rest_v[lo:hi].view(16, 3 * per, 3), X[:, :3, :3]))
                nn = torch.bmm(rest_n[lo:hi].view(16, 3 * per, 3), Xi[:, :3, :3].transpose(1, 2))
                world_n[lo:hi].view(16, 3 * per, 3).copy_(nn / nn.norm(dim=2, keepdim=True))
                ctx.refit_geometry(world_v, world_n)

            return events_ms(run)

        pose_all()  # the first refit derives the plan and blocks: not part of any figure
        ctx.synchronize()
        # the torch expression and the kernel agree to rounding (the kernel has the loader's bits, torch its own): the world arrays
        # are read right after the pose, before the caller's own refit makes the next read seed them from the records again
        xf = xforms(16)
        ctx.pose_objects(np.arange(16), xforms=xf, tree="refit")
        posed_v, posed_n = ctx.debug_read_world()
        call[0] -= 1  # the same transforms again
        torch_refit()
        ctx.synchronize()
        dv = float(np.abs(posed_v - world_v.cpu().numpy()).max())
        dn = float(np.abs(posed_n - world_n.cpu().numpy()).max())
        moved = float(np.abs(posed_v - sd.vertices).max())
        print(json.dumps({"scene": name, "max_abs_diff_vertices": dv, "max_abs_diff_normals": dn, "max_abs_motion": moved}), flush=True)
        assert moved > 1e-3 and dv < 1e-4 and dn < 1e-4, (moved, dv, dn)
        for r in range(args.rounds):
            row = {"scene": name, "triangles": int(sd.num_prims), "objects": 16, "triangles_per_object": per, "round": r}
            for what, fn in (("pose_all", pose_all), ("pose_one", pose_one), ("torch_refit", torch_refit)):
                ts = []
                for k in range(WARMUP + LAUNCHES):
                    t = fn()
                    if k >= WARMUP:
                        ts.append(t)
                row[what] = _stat(ts)
            print(json.dumps(row), flush=True)
            out.append(row)
        ctx.close()
        del rest_v, rest_n, world_v, world_n
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "pose_times.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
