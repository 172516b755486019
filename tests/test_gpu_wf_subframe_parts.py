"""The wavefront sub-frame pipelines (RDH_PT_WF_SUBFRAMES) give the same frame whatever their number and whatever the
hardware queues their streams land on.

Every pipeline launches the whole resident grid and its workgroups take their share of the work by ticket, in the order they
become resident (kernels_wave.h, workgroupTicket), so the work each wave does depends on timing.  The frame must not.  The pipeline
count (RADISH_WF_PARTS) and the queue count (GPU_MAX_HW_QUEUES) are read once per process, so each combination renders BASELINE
config 3 (teapots, 1920x1080, 8 bounces, material sort) in a child process of its own: one after another, each under its own time
limit, stopping at the first failure.  Each child renders the frame twice: with the ordinary literal-class lists, and with lists
cut to 4 entries (RDH_PT_WF_SMALL_LISTS), which leaves entries for the ticketed first round and the ordinary queues.  Images
and work counters must be bit-identical across all children, and a strided sample must equal the oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, DEPTH, LOOPER = 1920, 1080, 8, 3
CHILD_TIMEOUT = 300

CHILD = r"""
import json, sys
import numpy as np
import torch
from radish_pt_amd import api, scenes

out = sys.argv[1]
W, H, depth, looper = (int(v) for v in sys.argv[2:6])
ctx = api.Context(0)
ctx.set_partition(0, 1, 64)
ctx.upload_scene(scenes.teapots())
ctx.set_camera(scenes.teapots_camera(W, H))
base = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES | api.RDH_PT_COUNT
counters = {}
for name, flags in (("lists", base), ("small_lists", base | api.RDH_PT_WF_SMALL_LISTS)):
    d = torch.zeros(W * H, 3, device="cuda")
    i = torch.zeros(W * H, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, looper, depth, flags)
    np.save(f"{out}/{name}_direct.npy", d.cpu().numpy())
    np.save(f"{out}/{name}_indirect.npy", i.cpu().numpy())
    counters[name] = {k: int(v) for k, v in ctx.counters().items()}
ctx.close()
with open(f"{out}/counters.json", "w") as f:
    json.dump(counters, f)
"""


def _render(tmp_path, parts, queues):
    out = tmp_path / f"parts{parts}_queues{queues}"
    out.mkdir()
    env = dict(os.environ, RADISH_WF_PARTS=str(parts), GPU_MAX_HW_QUEUES=str(queues))
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), str(W), str(H), str(DEPTH), str(LOOPER)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, f"parts={parts} queues={queues}: exit {r.returncode}\n{r.stderr[-3000:]}"
    with open(out / "counters.json") as f:
        counters = json.load(f)
    return {name: (np.load(out / f"{name}_direct.npy"), np.load(out / f"{name}_indirect.npy"), counters[name])
            for name in ("lists", "small_lists")}


def test_subframe_parts_and_queues_agree(tmp_path):
    from radish_pt_amd import scenes

    ref = None
    for queues in (1, 2):
        for parts in (1, 2, 3):
            got = _render(tmp_path, parts, queues)  # a failure ends the sequence here
            if ref is None:
                ref = got["lists"]
                assert ref[2]["closestRays"] + ref[2]["anyRays"] > 20_000_000
            for name, (d, i, ct) in got.items():
                what = f"parts={parts} queues={queues} {name}"
                assert_bit_equal(d, ref[0], f"{what}: direct")
                assert_bit_equal(i, ref[1], f"{what}: indirect")
                assert ct == ref[2], what
    sd = scenes.teapots()
    cam = scenes.teapots_camera(W, H)
    ref_d = np.zeros((W * H, 3), np.float32)
    ref_i = np.zeros((W * H, 3), np.float32)
    idx, _ = oracle_path_trace_mt(sd, cam, ref_d, ref_i, 0, LOOPER, DEPTH, stride=97)
    assert_bit_equal(ref[0][idx], ref_d[idx], "sub-frame frame vs oracle sample, direct")
    assert_bit_equal(ref[1][idx], ref_i[idx], "sub-frame frame vs oracle sample, indirect")
