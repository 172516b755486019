#!/usr/bin/env python3
"""What a sample costs when several share one wavefront pass (rdh_path_trace_samples).

Per case, in ONE process, after warm-up of every variant, the variants are timed in turn, round after round (A B1 B2 ... A B1
B2 ...), so that whatever else the machine does falls on all of them alike:
  loop          A: the host loop, one path_trace call per sample
  spp1 .. spp16 B: one path_trace_samples call with samples_per_pass 1, 2, 4, 8, 16 (values above the case's sample count
                are the same call as the count itself and are left out)
  persistent    config 1 only: the looped persistent kernel, what RDH_PT_AUTO picks for that scene
Every figure is ms PER SAMPLE: device events around `reps` back-to-back images of the case's sample count on the context's
stream, ended by a synchronise, divided by reps x samples.  Per variant: median [min, max] over the rounds; the spread of A is the
yardstick for every difference.  Before timing, each variant's image is compared with the loop's bit for bit.

Cases: config 1 (Cornell 400x400, depth 4, 16 spp, WAVEFRONT | SORT_MATERIAL) and config 3 (teapots 1920x1080, depth 8, 8 spp,
WAVEFRONT | SORT_MATERIAL | WF_SUBFRAMES).  GPU_MAX_HW_QUEUES and RADISH_WF_PARTS are left as the environment sets them and
printed.  --out DIR appends the raw lines to DIR/bench_ab.txt."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", default="config1,config3")
    ap.add_argument("--label", default="", help="a word for the raw lines (e.g. the build of the library under RADISH_HIP_LIB)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from radish_pt_amd import api, scenes

    if not torch.cuda.is_available():
        sys.exit("samples_times.py needs a HIP device: there is nothing to time without one")
    wf = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL
    cases = {
        "config1": dict(scene=scenes.cornell, cam=scenes.cornell_camera, W=400, H=400, depth=4, spp=16, reps=8, flags=wf, persistent=True),
        "config3": dict(scene=scenes.teapots, cam=scenes.teapots_camera, W=1920, H=1080, depth=8, spp=8, reps=2,
                        flags=wf | api.RDH_PT_WF_SUBFRAMES, persistent=False),
    }
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# samples_times.py {args.label} library={os.path.basename(api.HIP_LIB_PATH)} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')} "
         f"RADISH_WF_PARTS={os.environ.get('RADISH_WF_PARTS', 'unset')} rounds={args.rounds} device={torch.cuda.get_device_name(0)}")
    for name in args.cases.split(","):
        cs = cases[name]
        W, H, depth, spp, reps, flags = cs["W"], cs["H"], cs["depth"], cs["spp"], cs["reps"], cs["flags"]
        ctx = api.Context(0)
        ctx.upload_scene(cs["scene"]())
        ctx.set_camera(cs["cam"](W, H))
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")

        def loop(fl):
            def run():
                for s in range(spp):
                    ctx.path_trace(d, i, s, s, depth, fl)
            return run

        def batched(b):
            return lambda: ctx.path_trace_samples(d, i, 0, 0, spp, depth, flags, samples_per_pass=b)

        variants = [("loop", loop(flags))] + [(f"spp{b}", batched(b)) for b in (1, 2, 4, 8, 16) if b <= spp]
        if cs["persistent"]:
            variants.append(("persistent", loop(api.RDH_PT_PERSISTENT)))
        # results first: every variant's image against the loop's, bit for bit (and warm-up of every shape: two more runs each)
        ref = None
        for vn, run in variants:
            run()
            ctx.synchronize()
            got = (d.cpu().numpy().view(np.uint32).copy(), i.cpu().numpy().view(np.uint32).copy())
            if ref is None:
                ref = got
            same = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
            emit(f"CHECK {name} {vn} bit_equal_to_loop {same}")
            if not same:
                sys.exit(f"{name} {vn}: the image differs from the loop's")
            for _ in range(2):
                run()
            ctx.synchronize()
        times = {vn: [] for vn, _ in variants}
        stream = torch.cuda.current_stream()
        for r in range(args.rounds):
            for vn, run in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(reps):
                    run()
                b.record(stream)
                b.synchronize()
                ms = a.elapsed_time(b) / (reps * spp)
                times[vn].append(ms)
                emit("SAMPLES_TIMES " + json.dumps({"label": args.label, "case": name, "variant": vn, "round": r, "ms_per_sample": round(ms, 4),
                                                    "samples": spp, "reps": reps}))
        for vn, _ in variants:
            ts = times[vn]
            emit(f"SUMMARY {args.label} {name} {vn:<10} ms/sample median {statistics.median(ts):.4f} [min {min(ts):.4f}, max {max(ts):.4f}] n={len(ts)}")
        ctx.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_ab.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
