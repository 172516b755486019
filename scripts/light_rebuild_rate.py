#!/usr/bin/env python3
"""Moving emissive geometry: what rebuilding the light sampler on the device costs next to the host path it replaces.

Per scene (Cornell: 2 lights; teapots with a 4x8 / 16x32 emissive grid: 66 / 1 026 lights), with the scene's own vertices:
rdh_scene_rebuild_lights (hipEvents on the context's stream, warm, best of 5) and the host path for a caller whose vertices live on
the device (wall clock, best of 3): vertices device -> host, rdh_build_light_list, rdh_build_alias_table, and the table's way back
through a pinned buffer.  Then rdh_build_alias_table_device against rdh_build_alias_table on 1 M synthetic values.  One JSON line
per row; --out DIR also writes them to DIR/light_rebuild_rate.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from radish_pt_amd import api, hostlib, scenes  # noqa: E402


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


def _wall_ms(fn, reps=3):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) * 1e3)
    return best


def run(name, sd):
    ctx = api.Context(0)
    row = {"scene": name, "triangles": int(sd.num_prims), "lights": int(len(sd.light_sampler))}
    ctx.upload_scene(sd)
    v = torch.from_numpy(sd.vertices).cuda()
    ctx.rebuild_lights(sd.env_power)
    ctx.synchronize()
    assert np.array_equal(ctx.debug_read_lights(0), sd.light_sampler), "the rebuilt table is not the host's"
    row["rebuild_lights_ms"] = _events_ms(lambda: ctx.rebuild_lights(sd.env_power))
    stage = torch.empty(len(sd.light_sampler), 2, dtype=torch.int32).pin_memory()
    dst = torch.empty(len(sd.light_sampler), 2, dtype=torch.int32, device="cuda")
    parts = {}

    def host_path():
        t0 = time.perf_counter()
        hv = v.cpu().numpy()
        t1 = time.perf_counter()
        _, _, power = hostlib.build_light_list(hv, sd.material_ids, sd.materials)
        if sd.env_map_tex_id >= 0:
            power = np.concatenate([power, np.array([sd.env_power], np.float32)]).astype(np.float32)
        t2 = time.perf_counter()
        table, _ = hostlib.build_alias_table(power)
        t3 = time.perf_counter()
        stage.numpy().view(np.uint8).reshape(-1)[:] = table.view(np.uint8)
        dst.copy_(stage, non_blocking=True)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        parts.update(vertices_d2h_ms=(t1 - t0) * 1e3, build_light_list_ms=(t2 - t1) * 1e3, build_alias_table_ms=(t3 - t2) * 1e3,
                     staged_copy_ms=(t4 - t3) * 1e3)

    row["host_path_wall_ms"] = _wall_ms(host_path)
    row["host_path_parts_last_run"] = dict(parts)
    row["host_over_device"] = row["host_path_wall_ms"] / row["rebuild_lights_ms"]
    ctx.close()
    return row


def run_table(n):
    ctx = api.Context(0)
    values = np.random.default_rng(21).exponential(1.0, n).astype(np.float32)
    dv = torch.from_numpy(values).cuda()
    table, total = ctx.build_alias_table_device(dv)
    ctx.synchronize()
    ht, hs = hostlib.build_alias_table(values)
    assert np.array_equal(table.cpu().numpy().view(np.uint8).reshape(-1), ht.view(np.uint8)), "device table != host table"
    assert total.cpu().numpy().view(np.uint32)[0] == np.array([hs], np.float32).view(np.uint32)[0]
    row = {"values": n, "build_alias_table_device_ms": _events_ms(lambda: ctx.build_alias_table_device(dv))}
    row["host_build_alias_table_wall_ms"] = _wall_ms(lambda: hostlib.build_alias_table(values))
    row["host_over_device"] = row["host_build_alias_table_wall_ms"] / row["build_alias_table_device_ms"]
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for name, sd in (("cornell", scenes.cornell()),
                     ("teapots_4x8", scenes.teapots(segments=24, bands=18, emissive_grid=(4, 8))),
                     ("teapots_16x32", scenes.teapots(emissive_grid=(16, 32)))):
        rows.append(run(name, sd))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(run_table(1_000_000))
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "light_rebuild_rate.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
