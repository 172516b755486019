#!/usr/bin/env python3
"""What replacing the triangle set on the device costs: Context.set_geometry with each builder against the only path
there was before it, Context.upload_scene of the edited SceneData, and against the same-count update it is built from.

Per scene (teapots with the 32 x 16 emissive grid, 100 364 + 1 024 triangles; the config-5 scene, about 1 M triangles, with the
same grid) the edit alternates between two descriptions: a quarter of the stand-ins removed (every fourth one), and all of them
back.  Per round and state, in turn and in one process:
  set_sah / set_lbvh  contexts that get set_geometry of the state's device arrays with that builder
  upload              a context that gets upload_scene of the prepared description: its host tree, light list and alias table were
                      built beforehand, OUTSIDE the figure (SceneData's constructor)
  update_sah / _lbvh  a context that holds the state's count already: update_geometry with that builder, then the list derivation
                      at the same count (build_light_list_device + rebuild_lights), which walk the same arrays
Each figure is an event pair on the stream around the call(s) and the host's wall time for them plus the wait for the stream,
reported as median [min, max] in ms.  After every group the contexts render a frame: set_sah's must be bit-equal to upload's,
set_lbvh's to update_lbvh's.  --out DIR writes the raw lines to DIR/bench_ab.txt."""
import argparse
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

    from radish_pt_amd import api, scenes

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
        full = scenes.teapots(segments=segments, bands=bands, emissive_grid=(16, 32))
        per = segments * bands * 2
        n = full.num_prims
        gone = np.zeros(n, bool)
        for k in range(0, 16, 4):  # a quarter of the stand-ins
            gone[12 + per * k:12 + per * (k + 1)] = True
        keep = np.flatnonzero(~gone)
        t0 = time.perf_counter()
        removed = scenes.SceneData(full.name + "_removed", full.vertices.reshape(n, 9)[keep].reshape(-1, 3),
                                   full.normals.reshape(n, 9)[keep].reshape(-1, 3), full.texcoords.reshape(n, 6)[keep].reshape(-1, 2),
                                   full.material_ids[keep], full.materials)
        emit({"scene": name, "triangles_full": int(n), "triangles_removed": int(removed.num_prims),
              "host_description_s": round(time.perf_counter() - t0, 2), "note": "host tree and tables of the removed state: outside every figure"})
        cam = scenes.teapots_camera(W, H)
        states = {"removed": removed, "full": full}
        dev = {k: tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
                        (s.vertices.reshape(-1), s.normals.reshape(-1), s.texcoords.reshape(-1), s.material_ids)) for k, s in states.items()}
        mats = torch.from_numpy(np.frombuffer(full.materials.tobytes(), np.uint8).copy()).cuda()
        setters = {b: api.Context(0) for b in ("sah", "lbvh")}
        up = api.Context(0)
        same = {k: api.Context(0) for k in states}  # hold the state's count already
        for c in list(setters.values()) + [up]:
            c.upload_scene(full)
            c.set_camera(cam)
        for k, c in same.items():
            c.upload_scene(states[k])
            c.set_camera(cam)
        for b, c in setters.items():  # warm: every workspace grown, the removed state seen once
            for k in ("removed", "full"):
                c.set_geometry(*dev[k], builder=b)
        for k, c in same.items():
            for b in ("sah", "lbvh"):
                c.update_geometry(dev[k][0], builder=b)
            c.build_light_list_device(dev[k][0], dev[k][3], mats)
            c.rebuild_lights()
            c.synchronize()
        ts = {}
        for r in range(args.rounds):
            for k, sd in states.items():
                row = {"scene": name, "round": r, "state": k, "triangles": int(sd.num_prims), "lights": int(sd.num_lights)}
                frames = {}
                for b, c in setters.items():
                    e, w = timed(c, lambda: c.set_geometry(*dev[k], builder=b))
                    row[f"set_{b}_event_ms"], row[f"set_{b}_wall_ms"] = round(e, 4), round(w, 4)
                    frames[f"set_{b}"] = frame(c)
                e, w = timed(up, lambda: up.upload_scene(sd))
                up.set_camera(cam)
                row["upload_event_ms"], row["upload_wall_ms"] = round(e, 4), round(w, 4)
                frames["upload"] = frame(up)
                y = same[k]
                for b in ("sah", "lbvh"):
                    e, w = timed(y, lambda: (y.update_geometry(dev[k][0], builder=b),
                                             y.build_light_list_device(dev[k][0], dev[k][3], mats), y.rebuild_lights()))
                    row[f"update_{b}_event_ms"], row[f"update_{b}_wall_ms"] = round(e, 4), round(w, 4)
                    frames[f"update_{b}"] = frame(y)
                assert np.array_equal(frames["set_sah"], frames["upload"]), f"{name} round {r} {k}: set_geometry(sah) and upload differ"
                assert np.array_equal(frames["set_sah"], frames["update_sah"]), f"{name} round {r} {k}: sah frames differ"
                assert np.array_equal(frames["set_lbvh"], frames["update_lbvh"]), f"{name} round {r} {k}: lbvh frames differ"
                row["frames_bit_equal"] = True
                for key, val in row.items():
                    if key.endswith("_ms"):
                        ts.setdefault((k, key), []).append(val)
                emit(row)
        for k in states:
            summary = {"scene": name, "state": k, "triangles": int(states[k].num_prims), "rounds": args.rounds}
            for (kk, key), vals in ts.items():
                if kk == k:
                    summary[key] = _stat(vals)
            emit(summary)
        for c in list(setters.values()) + [up] + list(same.values()):
            c.close()
        del dev
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_ab.txt"), "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
