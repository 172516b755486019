#!/usr/bin/env python3
"""What an adaptive pass costs (rdh_path_trace_adaptive), and how its cost follows the number of requested samples T.

Per case, in ONE process, after warm-up of every variant, the variants are timed in turn, round after round (A B C D A B C D ...),
so that whatever else the machine does falls on all of them alike:
  samples4        A: rdh_path_trace_samples(numSamples = 4, samplesPerPass = 4): 4 samples of every pixel in one whole-frame pass
  adaptive_all    B: the same 4 samples of every pixel through a request plane of 4s over counts of 0.  B - A is the price of the
                  list (count, scan, scatter, owner loads), the blocking read of T, and the pixel-major slot order
  adaptive_half   C: 4 samples on the 8x8 blocks adaptive_plan picks after 8 uniform samples at a threshold searched (bisection over
  adaptive_tenth  D: the GPU plan itself) so that about a half / a tenth of the blocks are active; counts of 8 there
Every figure is ms PER CALL: device events around `reps` back-to-back calls on the context's stream (the adaptive entry's own
synchronisation included: it happens between the events), ended by a synchronise, divided by reps.  Per variant: median [min, max]
over the rounds, and T; the spread of A is the yardstick for every difference.  Before timing, B's images are compared with A's bit
for bit.  The count planes are restored before every adaptive call (one small device copy, inside the timed region of B, C and D).

Cases: config 1 (Cornell 400x400, depth 4) and config 3 (teapots 1920x1080, depth 8), both WAVEFRONT | SORT_MATERIAL.
--out DIR appends the raw lines to DIR/bench_ab.txt.
--only VARIANT --calls N runs nothing but N calls of one variant (samples4 or adaptive_all) and times nothing: the process to put
under a kernel trace, so that the trace's per-kernel totals are that variant's (profiles/adaptive/trace_*.txt)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

R = 4  # samples per requested pixel in every variant


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", default="config1,config3")
    ap.add_argument("--label", default="")
    ap.add_argument("--only", default=None, choices=["samples4", "adaptive_all"])
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()

    import numpy as np
    import torch

    from radish_pt_amd import api, scenes

    if not torch.cuda.is_available():
        sys.exit("adaptive_times.py needs a HIP device: there is nothing to time without one")
    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL
    cases = {
        "config1": dict(scene=scenes.cornell, cam=scenes.cornell_camera, W=400, H=400, depth=4, reps=8),
        "config3": dict(scene=scenes.teapots, cam=scenes.teapots_camera, W=1920, H=1080, depth=8, reps=2),
    }
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# adaptive_times.py {args.label} library={os.path.basename(api.HIP_LIB_PATH)} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')} "
         f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}")
    for name in args.cases.split(","):
        cs = cases[name]
        W, H, depth, reps = cs["W"], cs["H"], cs["depth"], cs["reps"]
        P = W * H
        blocks = ((W + 7) // 8) * ((H + 7) // 8)
        ctx = api.Context(0)
        ctx.upload_scene(cs["scene"]())
        ctx.set_camera(cs["cam"](W, H))
        d, i = torch.zeros(P, 3, device="cuda"), torch.zeros(P, 3, device="cuda")
        counts = torch.zeros(P, dtype=torch.int32, device="cuda")
        if args.only:
            all4 = torch.full((P,), R, dtype=torch.int32, device="cuda")
            for _ in range(args.calls):
                if args.only == "samples4":
                    ctx.path_trace_samples(d, i, 0, 0, R, depth, flags, samples_per_pass=R)
                else:
                    counts.zero_()
                    ctx.path_trace_adaptive(d, i, counts, all4, 0, depth, flags)
            ctx.synchronize()
            emit(f"ONLY {name} {args.only} calls {args.calls}")
            ctx.close()
            continue

        # the plans: 8 uniform samples with moments, then the threshold at which about `share` of the blocks are active
        m8 = torch.zeros(P, 2, device="cuda")
        for _ in range(2):  # (two passes of 4: eight samples of a 1080p frame are more slots than one pass holds)
            ctx.path_trace_adaptive(d, i, counts, torch.full((P,), 4, dtype=torch.int32, device="cuda"), 0, depth, flags, moments=m8)
        c8 = counts.clone()

        def plan_for(share):
            lo, hi, best = 0.0, 4.0, None
            for _ in range(24):
                thr = 0.5 * (lo + hi)
                req = torch.zeros(P, dtype=torch.int32, device="cuda")
                st = ctx.adaptive_plan(c8, m8, req, 0, 1 << 20, R, thr)
                if best is None or abs(st["activeBlocks"] - share * blocks) < abs(best[1]["activeBlocks"] - share * blocks):
                    best = (req, st, thr)
                if st["activeBlocks"] > share * blocks:
                    lo = thr
                else:
                    hi = thr
            return best

        planes = {"adaptive_all": (torch.full((P,), R, dtype=torch.int32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda"))}
        for vn, share in (("adaptive_half", 0.5), ("adaptive_tenth", 0.1)):
            req, st, thr = plan_for(share)
            planes[vn] = (req, c8)
            emit(f"PLAN {name} {vn} threshold {thr:.6f} " + json.dumps(st) + f" blocks {blocks}")

        def adaptive(vn):
            req, start = planes[vn]

            def run():
                counts.copy_(start)
                return ctx.path_trace_adaptive(d, i, counts, req, 0, depth, flags)
            return run

        def samples():
            ctx.path_trace_samples(d, i, 0, 0, R, depth, flags, samples_per_pass=R)
            return P * R

        variants = [("samples4", samples)] + [(vn, adaptive(vn)) for vn in ("adaptive_all", "adaptive_half", "adaptive_tenth")]
        traced, ref = {}, None
        for vn, run in variants:  # results first (A and B give one image), and warm-up of every shape: two more runs each
            traced[vn] = run()
            ctx.synchronize()
            if vn in ("samples4", "adaptive_all"):
                got = (d.cpu().numpy().view(np.uint32).copy(), i.cpu().numpy().view(np.uint32).copy())
                ref = ref or got
                same = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
                emit(f"CHECK {name} {vn} bit_equal_to_samples4 {same}")
                if not same:
                    sys.exit(f"{name} {vn}: the image differs from rdh_path_trace_samples'")
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
                ms = a.elapsed_time(b) / reps
                times[vn].append(ms)
                emit("ADAPTIVE_TIMES " + json.dumps({"label": args.label, "case": name, "variant": vn, "round": r, "ms_per_call": round(ms, 4),
                                                     "T": traced[vn], "reps": reps}))
        for vn, _ in variants:
            ts = times[vn]
            med = statistics.median(ts)
            emit(f"SUMMARY {args.label} {name} {vn:<14} T {traced[vn]:>9} ms/call median {med:.4f} [min {min(ts):.4f}, max {max(ts):.4f}] "
                 f"ns/sample {1e6 * med / traced[vn]:.2f} n={len(ts)}")
        ctx.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_ab.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
