#!/usr/bin/env python3
"""What editing a texture or the environment map on the device costs: Context.set_texture against the only path there
was before it, Context.upload_scene of the edited SceneData.

Scenes: cornell_textured (780 triangles) with an environment map of 64 x 32, 512 x 256 and 2048 x 1024 pixels, and teapots
(100 364 triangles) with one of 512 x 256.  Each scene also carries a plain texture of the environment map's size that no material
names, so that a plain edit of the same texel count can be timed beside the environment edit.  Two images of each (the sun in two
places) are set in turn.

Context A gets the edits, context B the upload of the edited description, whose host tables (environment alias table, light alias
table) were built beforehand: that work is not in B's figure; the host's build_envmap_sampler alone is timed beside it.  A and B go
in turn, `--rounds` times over in one process after one round that is not counted (the first environment edit of a scene allocates
its workspace and sends the row factors); each figure is an event pair on the stream around the call and the host's wall time for
the call plus the wait for the stream, reported as median [min, max] in ms.  After every pair both contexts render a frame, which
must be bit-equal.  --out DIR writes the raw lines to DIR/bench_ab.txt."""
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


def sky(w, h, sun):
    """scenes._sky with the sun at (u, v) = sun."""
    import numpy as np

    v = (np.arange(h, dtype=np.float64) + 0.5) / h
    u = (np.arange(w, dtype=np.float64) + 0.5) / w
    V, U = np.meshgrid(v, u, indexing="ij")
    top = np.stack([0.25 + 0.3 * (1 - V), 0.4 + 0.35 * (1 - V), 0.7 + 0.3 * (1 - V)], -1) * (V < 0.5)[..., None]
    ground = np.stack([0.12 + 0 * V, 0.1 + 0 * V, 0.08 + 0 * V], -1) * (V >= 0.5)[..., None]
    s = 40.0 * np.exp(-(((U - sun[0]) / 0.03) ** 2 + ((V - sun[1]) / 0.04) ** 2))
    return (top + ground + s[..., None] * np.array([1.0, 0.9, 0.7])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated case names (cornell_64x32, cornell_512x256, cornell_2048x1024, teapots_512x256)")
    ap.add_argument("--append", action="store_true", help="add to DIR/bench_ab.txt instead of replacing it")
    args = ap.parse_args()

    import numpy as np
    import torch

    from radish_pt_amd import api, hostlib, scenes

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

    def with_maps(sd, plain_id, plain, env):
        """sd with the two textures replaced and the fields of SceneData that depend on the environment map derived again (the
        tree and the emitter list do not)."""
        e = copy.copy(sd)
        e.textures = list(sd.textures)
        e.textures[plain_id], e.textures[sd.env_map_tex_id] = plain, env
        e.env_map_sampler, s = hostlib.build_envmap_sampler(env, env.shape[1], env.shape[0])
        e.env_power = np.float32(s)
        power = np.concatenate([sd.light_power, np.array([s], np.float32)]).astype(np.float32)
        e.light_sampler, total = hostlib.build_alias_table(power)
        e.sum_light_power_inv = np.float32(1.0) / np.float32(total)
        return e

    def frame(ctx):
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.path_trace(d, i, 0, 3, DEPTH, api.RDH_PT_PERSISTENT)
        ctx.synchronize()
        return np.concatenate([d.cpu().numpy(), i.cpu().numpy()]).view(np.uint32)

    cases = [("cornell", 64, 32), ("cornell", 512, 256), ("cornell", 2048, 1024), ("teapots", 512, 256)]
    only = set(args.only.split(",")) if args.only else None
    for base, w, h in cases:
        name = f"{base}_{w}x{h}"
        if only is not None and name not in only:
            continue
        envs = [sky(w, h, (0.3, 0.22)), sky(w, h, (0.62, 0.31))]
        plains = [np.ascontiguousarray(e[::-1] * np.float32(0.5)) for e in envs]
        src = scenes.cornell_textured(env=False) if base == "cornell" else scenes.teapots()
        cam = scenes.cornell_camera(W, H) if base == "cornell" else scenes.teapots_camera(W, H)
        tex = list(src.textures) + [plains[0], envs[0]]
        plain_id, env_id = len(tex) - 2, len(tex) - 1
        sd = scenes.SceneData(name, src.vertices, src.normals, src.texcoords, src.material_ids, src.materials, tex, env_id)
        states = [sd, with_maps(sd, plain_id, plains[1], envs[1])]
        assert states[0].env_power.tobytes() == with_maps(sd, plain_id, plains[0], envs[0]).env_power.tobytes()
        d_envs, d_plains = [torch.from_numpy(e).cuda() for e in envs], [torch.from_numpy(p).cuda() for p in plains]
        a, b = api.Context(0), api.Context(0)
        for c in (a, b):
            c.upload_scene(sd)
            c.set_camera(cam)
        ts = {}
        for r in range(-1, args.rounds):  # round -1 warms every shape up and is not counted
            k = (r + 2) % 2
            ee, we = timed(a, lambda: a.set_texture(env_id, d_envs[k]))
            ep, wp = timed(a, lambda: a.set_texture(plain_id, d_plains[k]))
            eu, wu = timed(b, lambda: b.upload_scene(states[k]))
            b.set_camera(cam)
            t0 = time.perf_counter()
            hostlib.build_envmap_sampler(envs[k], w, h)
            host = (time.perf_counter() - t0) * 1e3
            fa, fb = frame(a), frame(b)
            assert np.array_equal(fa, fb), f"{name} round {r}: frames differ"
            assert a.env_power().tobytes() == states[k].env_power.tobytes(), f"{name} round {r}: env_power differs"
            if r < 0:
                continue
            for key, val in (("env_edit_event", ee), ("env_edit_wall", we), ("plain_edit_event", ep), ("plain_edit_wall", wp),
                             ("upload_event", eu), ("upload_wall", wu), ("host_envmap_sampler_wall", host)):
                ts.setdefault(key, []).append(val)
            emit({"scene": name, "triangles": int(sd.num_prims), "pixels": w * h, "round": r, "env_edit_event_ms": round(ee, 4),
                  "env_edit_wall_ms": round(we, 4), "plain_edit_event_ms": round(ep, 4), "plain_edit_wall_ms": round(wp, 4),
                  "upload_event_ms": round(eu, 4), "upload_wall_ms": round(wu, 4), "host_envmap_sampler_wall_ms": round(host, 4),
                  "frames_bit_equal": True})
        summary = {"scene": name, "triangles": int(sd.num_prims), "pixels": w * h, "rounds": args.rounds}
        for key, vals in ts.items():
            summary[f"{key}_ms"] = _stat(vals)
        emit(summary)
        for c in (a, b):
            c.close()
        del d_envs, d_plains
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_ab.txt"), "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
