"""Summarise a `rocprofv3 --kernel-trace --output-format csv` run of the wavefront path tracer.

Per frame (first k_wf_raygen to last k_wf_finish): the frame span, the hardware queue and stream of every sub-frame pipeline's
dispatches, the per-launch durations of k_wf_trace / k_wf_shade, and the time during which stages of two different pipelines
ran at the same moment.  Usage: python scripts/wf_trace_summary.py <run_kernel_trace.csv> [frames to print]
"""
import csv
import sys
from collections import defaultdict


def short(name):
    for k in ("k_wf_raygen", "k_wf_trace", "k_wf_shade", "k_wf_finish"):
        if k in name:
            return k
    return None


def main():
    rows = []
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if k:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, int(r["Queue_Id"]), int(r["Stream_Id"]), int(r["Dispatch_Id"])))
    rows.sort(key=lambda x: x[5])
    frames, cur = [], None
    for x in rows:  # a frame opens with its run of k_wf_raygen dispatches
        if x[2] == "k_wf_raygen" and (cur is None or cur[-1][2] != "k_wf_raygen"):
            cur = []
            frames.append(cur)
        if cur is not None:
            cur.append(x)
    show = int(sys.argv[2]) if len(sys.argv) > 2 else len(frames)
    spans = []
    for n, fr in enumerate(frames):
        t0 = min(x[0] for x in fr if x[2] == "k_wf_raygen")
        t1 = max(x[1] for x in fr if x[2] == "k_wf_finish") if any(x[2] == "k_wf_finish" for x in fr) else None
        if t1 is None:
            continue
        spans.append((t1 - t0) / 1e6)
        pipes = defaultdict(list)  # pipeline = stream
        for x in fr:
            pipes[x[4]].append(x)
        # overlap: time during which stages (trace / shade) of at least two pipelines were running
        ev = []
        for s, xs in pipes.items():
            for x in xs:
                if x[2] in ("k_wf_trace", "k_wf_shade"):
                    ev += [(x[0], 1, s), (x[1], -1, s)]
        ev.sort()
        live, both, last = defaultdict(int), 0, None
        for t, d, s in ev:
            if last is not None and sum(1 for v in live.values() if v > 0) >= 2:
                both += t - last
            live[s] += d
            last = t
        if n < show:
            print(f"frame {n}: span {(t1 - t0) / 1e6:.3f} ms, stages of two pipelines at once {both / 1e6:.3f} ms")
            for s, xs in sorted(pipes.items()):
                qs = sorted({x[3] for x in xs})
                tr = [(x[1] - x[0]) / 1e3 for x in xs if x[2] == "k_wf_trace"]
                sh = [(x[1] - x[0]) / 1e3 for x in xs if x[2] == "k_wf_shade"]
                print(f"  stream {s} queue {qs}: {len(xs)} dispatches, "
                      f"{min(x[0] for x in xs) / 1e6 - t0 / 1e6:.3f}..{max(x[1] for x in xs) / 1e6 - t0 / 1e6:.3f} ms")
                print("    k_wf_trace us: " + " ".join(f"{v:.0f}" for v in tr))
                print("    k_wf_shade us: " + " ".join(f"{v:.0f}" for v in sh))
    if spans:
        spans.sort()
        print(f"{len(spans)} frames: span min {spans[0]:.3f} ms, median {spans[len(spans) // 2]:.3f} ms, max {spans[-1]:.3f} ms")


if __name__ == "__main__":
    main()
