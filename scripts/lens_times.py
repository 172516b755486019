#!/usr/bin/env python3
"""What the lens costs a frame (rdh_set_lens), and whether stage 0 of a lens frame should still go as packets.

Cases: the benchmark's frame (teapots 1920x1080, 8 bounces, WAVEFRONT | SORT_MATERIAL | WF_SUBFRAMES), each lens variant once with
stage-0 packets and once with RDH_PT_NO_PACKETS, and BASELINE config 2's frame (Cornell 1920x1080, 8 bounces, PERSISTENT).
Lens variants: off; disk at three radii chosen so that the circle of confusion at the scene's farthest vertex along the view (the
room's back wall) is about 0 (0.01), 8 and 64 pixels with the focus at three quarters of that depth; a 64x64 mask (a hexagonal
aperture) at the middle radius.  For a point at depth z and the focus at depth f the blur's diameter is
2 R |z - f| / (z f) at unit distance, and a pixel is 2 tan(fovY) / H there, so R = coc * z * f * tan(fovY) / (|z - f| * H).

In ONE process per case, after a warm-up of every variant, the variants are timed in turn, round after round (A B C ... A B C ...),
so that whatever else the machine does falls on all of them alike.  A figure is ms per frame: device events around `reps`
back-to-back rdh_path_trace calls, divided by reps.  Per variant: median [min, max] over the rounds; the spread of `off` is the
yardstick for every difference.

Also: the host time of rdh_set_lens(MASK) — luminances, alias table, the wait for the sum — for 16x16, 64x64 and 256x256 masks,
median of 7 calls each.  It is paid once per mask (and once per rdh_scene_set_texture on it), not per frame.

--out DIR writes the raw lines to DIR/lens_times.txt."""
import argparse
import json
import math
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

COCS = (("disk_coc0", 0.01), ("disk_coc8", 8.0), ("disk_coc64", 64.0))


def hexagon_mask(n):
    """n x n texels: 1 inside a regular hexagon inscribed in the square, 0 outside."""
    import numpy as np

    y, x = (np.mgrid[0:n, 0:n] + 0.5) / n * 2.0 - 1.0
    inside = (np.abs(y) <= math.sqrt(3.0) / 2.0) & (np.abs(y) + math.sqrt(3.0) * np.abs(x) <= math.sqrt(3.0))
    return np.repeat(inside[..., None], 3, axis=2).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", default="teapots_wavefront,cornell_persistent")
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from radish_pt_amd import api, scenes

    if not torch.cuda.is_available():
        sys.exit("lens_times.py needs a HIP device: there is nothing to time without one")
    wf = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES
    cases = {
        "teapots_wavefront": dict(scene=scenes.teapots, cam=scenes.teapots_camera, W=1920, H=1080, depth=8, reps=2,
                                  structures=(("packets", wf), ("no_packets", wf | api.RDH_PT_NO_PACKETS))),
        "cornell_persistent": dict(scene=scenes.cornell, cam=scenes.cornell_camera, W=1920, H=1080, depth=8, reps=3,
                                   structures=(("persistent", api.RDH_PT_PERSISTENT),)),
    }
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# lens_times.py {args.label} library={os.path.basename(api.HIP_LIB_PATH)} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')} "
         f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}")
    for name in args.cases.split(","):
        cs = cases[name]
        W, H, depth, reps = cs["W"], cs["H"], cs["depth"], cs["reps"]
        P = W * H
        sd = cs["scene"]()
        first_mask = len(sd.textures)  # the masks: three more textures that no material names (the upload takes the list as it stands)
        sd.textures = list(sd.textures) + [hexagon_mask(n) for n in (16, 64, 256)]
        pin = cs["cam"](W, H)
        eye, view = pin["position"].astype(np.float64), pin["view"].astype(np.float64)
        z = float(((sd.vertices.astype(np.float64) - eye) @ view).max())
        f = 0.75 * z
        tan = math.tan(math.radians(float(pin["fov"][1])))
        radius = {vn: coc * z * f * tan / (abs(z - f) * H) for vn, coc in COCS}
        emit(f"SETUP {name} back wall depth {z:.4f} focus {f:.4f} radii " + json.dumps({k: round(v, 6) for k, v in radius.items()}))

        def camera(r):
            cam = pin.copy()
            cam["lensRadius"], cam["focalDist"] = r, f
            return cam

        lens = [("off", "off", -1, camera(0.0))] + [(vn, "disk", -1, camera(radius[vn])) for vn, _ in COCS] + \
               [("mask64_coc8", "mask", first_mask + 1, camera(radius["disk_coc8"]))]
        ctx = api.Context(0)
        ctx.upload_scene(sd)
        ctx.set_camera(pin)
        d, i = torch.zeros(P, 3, device="cuda"), torch.zeros(P, 3, device="cuda")

        if name == args.cases.split(",")[0]:  # the table's build, once
            for k, n in enumerate((16, 64, 256)):
                ts = []
                for _ in range(7):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    ctx.set_lens("mask", first_mask + k)
                    ts.append(1e3 * (time.perf_counter() - t0))
                emit(f"TABLE_BUILD {n}x{n} entries {n * n} ms median {statistics.median(ts):.4f} [min {min(ts):.4f}, max {max(ts):.4f}] n=7")
            ctx.set_lens("off")

        variants = [(f"{ln}/{sn}", mode, tex, cam, flags) for sn, flags in cs["structures"] for ln, mode, tex, cam in lens]

        def run(v):
            _, mode, tex, cam, flags = v
            ctx.set_lens(mode, tex)
            ctx.set_camera(cam)
            return flags

        for v in variants:  # warm-up of every variant: three frames each
            flags = run(v)
            for it in range(3):
                ctx.path_trace(d, i, it, it, depth, flags)
            ctx.synchronize()
        times = {v[0]: [] for v in variants}
        stream = torch.cuda.current_stream()
        for r in range(args.rounds):
            for v in variants:
                flags = run(v)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for it in range(reps):
                    ctx.path_trace(d, i, it, (r * reps + it) % 10000, depth, flags)
                b.record(stream)
                b.synchronize()
                ms = a.elapsed_time(b) / reps
                times[v[0]].append(ms)
                emit("LENS_TIMES " + json.dumps({"label": args.label, "case": name, "variant": v[0], "round": r, "ms_per_frame": round(ms, 4),
                                                 "reps": reps}))
        for v in variants:
            ts = times[v[0]]
            emit(f"SUMMARY {args.label} {name} {v[0]:<24} ms/frame median {statistics.median(ts):.4f} [min {min(ts):.4f}, max {max(ts):.4f}] n={len(ts)}")
        ctx.set_lens("off")
        ctx.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "lens_times.txt"), "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
