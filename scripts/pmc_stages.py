#!/usr/bin/env python3
"""Per-STAGE counters of the wavefront frame from `rocprofv3 --pmc ... --output-format csv` runs of scripts/pmc_frames.py (one or more
passes, each in a directory of its own): the dispatches of a pass are split into frames at k_wf_raygen, the j-th k_wf_trace / k_wf_shade
of a frame is stage j, and every counter is averaged over the frames.  With a records file (scripts/wf_stage_records.py) the table
holds the stage's records beside its bytes, and for k_wf_shade the ratio of the written bytes to the bytes its stores hold:
continuing records x 112 B (six float4, rng, two queue entries), continuing = max(rayCount[k + 1], shadowCount[k]).
FETCH_SIZE / WRITE_SIZE are KiB as the profiler reports them (FETCH_SIZE tallies a 128-B request as 64 B: scripts/pmc_per_frame.py).
usage: pmc_stages.py <records file or -> <pass dir> [<pass dir> ...]"""
import collections, csv, glob, os, sys

records = {}
if sys.argv[1] != "-":
    for line in open(sys.argv[1]):
        if line.strip() and not line.startswith("#"):
            k, r, s = (int(v) for v in line.split())
            records[k] = (r, s)
acc = collections.defaultdict(lambda: collections.defaultdict(list))  # (kernel, stage) -> counter -> per-frame values
for root in sys.argv[2:]:
    for f in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        disp = collections.defaultdict(lambda: collections.defaultdict(float))
        names = {}
        for row in csv.DictReader(open(f)):
            i = int(row["Dispatch_Id"])
            names[i] = row["Kernel_Name"]
            disp[i][row["Counter_Name"]] += float(row["Counter_Value"])
        stage = None
        for i in sorted(disp):
            n = names[i]
            if "k_wf_raygen" in n:
                stage = {"k_wf_trace": 0, "k_wf_shade": 0}
            for kern in ("k_wf_trace", "k_wf_shade"):
                if kern in n and stage is not None:
                    for c, v in disp[i].items():
                        acc[(kern, stage[kern])][c].append(v)
                    stage[kern] += 1
counters = sorted({c for v in acc.values() for c in v})
for kern in ("k_wf_shade", "k_wf_trace"):
    stages = sorted(s for (k, s) in acc if k == kern)
    if not stages:
        continue
    frames = max(len(v) for s in stages for v in acc[(kern, s)].values())
    print(f"{kern}: mean per dispatch over {frames} frames")
    head = f"  {'stage':>5s} {'rays':>9s} {'shadow':>9s}" + "".join(f" {c:>16s}" for c in counters)
    if kern == "k_wf_shade" and records:
        head += f" {'held KiB':>10s} {'written/held':>12s}"
    print(head)
    tot = collections.defaultdict(float)
    for s in stages:
        r, sh = records.get(s, (0, 0))
        line = f"  {s:5d} {r:9d} {sh:9d}"
        for c in counters:
            v = acc[(kern, s)].get(c, [])
            m = sum(v) / len(v) if v else float("nan")
            tot[c] += m
            line += f" {m:16.0f}"
        if kern == "k_wf_shade" and records:
            cont = max(records.get(s + 1, (0, 0))[0], sh)
            held = cont * 112 / 1024
            w = acc[(kern, s)].get("WRITE_SIZE", [])
            line += f" {held:10.0f} " + (f"{(sum(w) / len(w)) / held:12.2f}" if w and held > 0 else f"{'-':>12s}")
        print(line)
    print(f"  {'all':>5s} {'':9s} {'':9s}" + "".join(f" {tot[c]:16.0f}" for c in counters))
