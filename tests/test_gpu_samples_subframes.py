"""rdh_path_trace_samples over the wavefront SUB-FRAME pipelines (RDH_PT_WF_SUBFRAMES): the sample groups are dealt to the
pipelines with their 8x8 blocks, each pipeline over its own workspace of B times the slots.

The pipeline count (RADISH_WF_PARTS) is read once per process, so the frames are rendered by one child process with three
pipelines.  Cornell at 512x256 is 2 048 blocks, the threshold at which sub-frames engage; block b belongs to pipeline b % 3, so
the pipelines hold 683, 683 and 682 blocks.  Depth 4, 3 samples from looper 9999 (the wrap lies inside), in passes of 3 and of
2 + 1, with the sibling-pair walks and without.  The child compares each against the looped path_trace with the same flags: images
and work counters bit for bit.  (The loop is pinned to the oracle by test_gpu_configs.py and test_gpu_wf_subframe_parts.py.)
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300  # seconds; the child takes a few (start-up, BVH upload, 4 x 3 wavefront frames of 131 072 pixels)

CHILD = r"""
import sys
import numpy as np
import torch
from helpers import assert_bit_equal
from radish_pt_amd import api, scenes

W, H, depth, samples, looper0 = 512, 256, 4, 3, 9999
ctx = api.Context(0)
ctx.set_partition(0, 1, 64)
ctx.upload_scene(scenes.cornell())
ctx.set_camera(scenes.cornell_camera(W, H))
base = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES | api.RDH_PT_COUNT
for walk, flags in (("pairs", base | api.RDH_PT_PAIRS), ("no_pairs", base | api.RDH_PT_NO_PAIRS)):
    ld, li = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    ctx.counters_reset()
    for s in range(samples):
        ctx.path_trace(ld, li, s, (looper0 + s) % 10000, depth, flags)
    want = ctx.counters()
    ld, li = ld.cpu().numpy(), li.cpu().numpy()
    assert ld.max() > 0 and li.max() > 0 and want["closestRays"] > samples * W * H, walk
    for spp in (3, 2):
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        ctx.counters_reset()
        ctx.path_trace_samples(d, i, 0, looper0, samples, depth, flags, samples_per_pass=spp)
        got = ctx.counters()
        print(f"{walk} samples_per_pass={spp}: counters {got}, the loop's {want}", flush=True)
        assert_bit_equal(d.cpu().numpy(), ld, f"{walk} samples_per_pass={spp}: direct")
        assert_bit_equal(i.cpu().numpy(), li, f"{walk} samples_per_pass={spp}: indirect")
        assert got == want, f"{walk} samples_per_pass={spp}: counters"
ctx.close()
"""


def test_samples_over_three_subframe_pipelines():
    env = dict(os.environ, RADISH_WF_PARTS="3")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.count("samples_per_pass=") == 4
