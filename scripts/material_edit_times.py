#!/usr/bin/env python3
"""What editing materials on the device costs: Context.set_materials against the only path there was before it,
Context.upload_scene of the edited SceneData.

Per scene (teapots with the 32 x 16 emissive grid, 100 364 + 1 024 triangles and 1 026 lights; the config-5 scene, about 1 M
triangles, with the same grid) three edits are timed:
  recolour  a non-emissive material gets another colour: records and shading classes only, no list rebuild
  half_off  every other emissive quad's material becomes Lambertian: the list, the alias table and the constants are derived again
  back_on   and Light again
Context A gets the edit, context B the upload of the edited description (whose light list and alias table were built on the host
beforehand: that work is not in B's figure).  The two are taken in turn, edit by edit, `--rounds` times over in one process; each
figure is an event pair on the stream around the call and the host's wall time for the call plus the wait for the stream, reported
as median [min, max] in ms.  After every pair both contexts render a frame, which must be bit-equal.  A third context gives the
yardstick of the same round: refit_geometry of the uploaded vertices followed by rebuild_lights, which walk the same arrays.
--out DIR writes the raw lines to DIR/bench_ab.txt."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
W, H, DEPTH = 256, 192, 4


def _stat(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-1m", action="store_true")
    ap.add_argument("--only-1m", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to DIR/bench_ab.txt instead of replacing it")
    args = ap.parse_args()

    import numpy as np
    import torch

    from radish_pt_amd import api, hostlib, layouts as L, scenes

    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))

    def timed(ctx, fn):
        """(event ms, wall ms): the call on the stream, and the call plus the wait for the stream on the host."""
        stream = torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return a.elapsed_time(b), wall

    def with_materials(sd, ids, mats):
        """sd with the materials replaced and the light fields of SceneData derived again (the tree does not depend on them)."""
        e = copy.copy(sd)
        e.materials = sd.materials.copy()
        e.materials[ids] = mats
        e.light_prim_ids, e.light_unit_radiance, e.light_power = hostlib.build_light_list(e.vertices, e.material_ids, e.materials)
        e.num_lights = len(e.light_prim_ids)
        e.light_sampler, s = hostlib.build_alias_table(e.light_power)
        e.sum_light_power_inv = np.float32(1.0) / np.float32(s)
        return e

    def frame(ctx):
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.path_trace(d, i, 0, 3, DEPTH, api.RDH_PT_PERSISTENT)
        ctx.synchronize()
        return np.concatenate([d.cpu().numpy(), i.cpu().numpy()]).view(np.uint32)

    todo = []
    if not args.only_1m:
        todo.append(("teapots", 64, 49))
    if not args.skip_1m:
        todo.append(("config5", 200, 156))
    for name, segments, bands in todo:
        sd = scenes.teapots(segments=segments, bands=bands, emissive_grid=(16, 32))
        assert sd.num_lights == 1026 and sd.env_map_tex_id < 0
        cam = scenes.teapots_camera(W, H)
        lights = np.flatnonzero(sd.materials["type"] == L.LIGHT).astype(np.int32)[1:]  # the quads'; the ceiling light stays
        half = lights[::2]
        dark = sd.materials[half].copy()
        dark["type"] = L.LAMBERTIAN
        tint = sd.materials[[4]].copy()  # the first stand-in's Lambertian
        tint["baseColor"] = (0.2, 0.3, 0.9)
        states = {  # edit -> (ids, materials, the description after it), applied in this order each round
            "recolour": (np.array([4], np.int32), tint),
            "half_off": (half, dark),
            "back_on": (half, sd.materials[half].copy()),
            "restore": (np.array([4], np.int32), sd.materials[[4]].copy()),
        }
        a, b, y = api.Context(0), api.Context(0), api.Context(0)
        for c in (a, b, y):
            c.upload_scene(sd)
            c.set_camera(cam)
        v = torch.from_numpy(sd.vertices).cuda()
        y.refit_geometry(v)  # the first refit derives the plan and blocks: not part of any figure
        y.rebuild_lights()
        y.synchronize()
        ts = {}
        for r in range(args.rounds):
            cur = sd
            for edit, (ids, mats) in states.items():
                cur = with_materials(cur, ids, mats)
                ea, wa = timed(a, lambda: a.set_materials(ids, mats))
                eb, wb = timed(b, lambda: b.upload_scene(cur))
                b.set_camera(cam)
                fa, fb = frame(a), frame(b)
                assert np.array_equal(fa, fb), f"{name} round {r} {edit}: frames differ"
                assert int(a.debug_read_lights(1).view(np.int32)[3]) == cur.num_lights
                if edit != "restore":
                    for key, val in (("edit_event", ea), ("edit_wall", wa), ("upload_event", eb), ("upload_wall", wb)):
                        ts.setdefault((edit, key), []).append(val)
                    emit({"scene": name, "triangles": int(sd.num_prims), "round": r, "edit": edit, "lights_after": int(cur.num_lights),
                          "edit_event_ms": round(ea, 4), "edit_wall_ms": round(wa, 4), "upload_event_ms": round(eb, 4),
                          "upload_wall_ms": round(wb, 4), "frames_bit_equal": True})
            ey, wy = timed(y, lambda: (y.refit_geometry(v), y.rebuild_lights()))
            ts.setdefault(("yardstick", "event"), []).append(ey)
            ts.setdefault(("yardstick", "wall"), []).append(wy)
            emit({"scene": name, "round": r, "refit_plus_rebuild_event_ms": round(ey, 4), "refit_plus_rebuild_wall_ms": round(wy, 4)})
        summary = {"scene": name, "triangles": int(sd.num_prims), "rounds": args.rounds}
        for (what, key), vals in ts.items():
            summary[f"{what}_{key}_ms"] = _stat(vals)
        emit(summary)
        for c in (a, b, y):
            c.close()
        del v
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_ab.txt"), "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
