"""k_gbuffer_persistent<.., PAIRS = true>: the G-buffer's lane-refill kernel over the sibling pairs.

The host picks it only for trees whose node arrays exceed 256 MiB, or with RADISH_GBUFFER_PAIRS=1 in the environment, which is read
once per process: so one child process with that variable set renders everything below (every call with RDH_PT_NO_PACKETS, the
lane-refill kernel), under a time limit of its own, and the parent compares what it saved.
  (a) the small teapots scene against the oracle: planes bit-equal, work counters equal — an ordinary camera over two frames, and an
      axis-aligned one whose centre row and column are literal-class rays, set aside for k_gbuffer_literal and traced in place;
  (b) a chain-shaped tree of 1 500 levels against the oracle: with the counters on, failed far children are stacked too and the
      stack outgrows its 8-entry LDS ring into the global strip, whose per-workgroup part the kernel's wrapper computes;
  (c) the full teapots frame, where there are more 8x8 blocks (32 400) than resident waves (at most 4 096) and a wave takes further
      chunks from the shared counter: pairs with and without the set-aside launch against one lane per pixel (no oracle at 2 M rays).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal, chain_scene, count_literal_primary_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
PLANES = ("albedo", "normal", "depth", "primId", "motion")
COUNTERS = ("closestRays", "nodeVisits", "triTests", "closestHits")


def _small_teapots():
    from radish_pt_amd import scenes

    return scenes.teapots(segments=12, bands=8, grid=2, emissive_grid=(4, 8))


def _cams_ordinary():
    from radish_pt_amd import hostlib

    return [hostlib.make_camera(150, 91, eye=(0.3 + 0.1 * f, 1.9, 7.4), rotation=(-91.5, -11.0, 0.0), fovy=19.0) for f in range(2)]


def _cam_axis():
    from radish_pt_amd import hostlib

    return hostlib.make_camera(151, 91, eye=(0.0, 1.0, 9.0), rotation=(-90.0, 0.0, 0.0), fovy=19.0)


def _cam_chain():
    from radish_pt_amd import hostlib

    return hostlib.make_camera(48, 32, eye=(0.2, 0.7, 4.5), rotation=(-90.0, 0.0, 0.0), fovy=19.5)


# name -> (scene, cameras of consecutive frames, flags beside RDH_PT_NO_PACKETS, counted?)
def _oracle_cases():
    from radish_pt_amd import api

    return {
        "teapots_count": ("teapots", _cams_ordinary(), 0, True),
        "teapots_plain": ("teapots", _cams_ordinary()[:1], 0, False),
        "axis_defer": ("teapots", [_cam_axis()], 0, True),
        "axis_in_place": ("teapots", [_cam_axis()], api.RDH_PT_NO_DEFER, True),
        "chain_count": ("chain", [_cam_chain()], 0, True),
        "chain_plain": ("chain", [_cam_chain()], 0, False),
    }


CHILD = r"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import test_gpu_gbuffer_pairs as T
from helpers import chain_scene
from radish_pt_amd import api, hostlib, scenes

out = sys.argv[1]
ctx = api.Context(0)
ctx.set_partition(0, 1, 64)

def render(cam, gb, flags):
    ctx.set_camera(cam)
    ctx.counters_reset()
    ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), flags | api.RDH_PT_NO_PACKETS)
    ctx.synchronize()
    f = gb.frameIdx
    planes = [gb.albedo.cpu().numpy(), gb.normal[f].cpu().numpy(), gb.depth[f].cpu().numpy(), gb.primId[f].cpu().numpy(),
              gb.motion.cpu().numpy()]
    return planes, {k: int(v) for k, v in ctx.counters().items()}

counters = {}
uploaded = None
for name, (scene, cams, flags, count) in T._oracle_cases().items():
    if scene != uploaded:
        ctx.upload_scene(T._small_teapots() if scene == "teapots" else chain_scene(1500))
        uploaded = scene
    w, h = int(cams[0]["resolution"][0]), int(cams[0]["resolution"][1])
    gb = api.GBuffer()
    gb.create(w, h)
    for f, cam in enumerate(cams):
        planes, ct = render(cam, gb, flags | (api.RDH_PT_COUNT if count else 0))
        np.savez(f"{out}/{name}_{f}.npz", **dict(zip(T.PLANES, planes)))
        counters[f"{name}_{f}"] = ct
        gb.update(cam)

# (c) the full frame: compared here (five planes of 2 M pixels per variant), the verdict saved
ctx.upload_scene(scenes.teapots(emissive_grid=(16, 32)))
W, H = 1920, 1080
full = {}
for cname, cam in (("bench", scenes.teapots_camera(W, H)),
                   ("axis", hostlib.make_camera(W - 1, H - 1, eye=(0.0, 1.5, 9.0), rotation=(-90.0, 0.0, 0.0), fovy=19.0))):
    w, h = int(cam["resolution"][0]), int(cam["resolution"][1])
    got = {}
    for name, flags in (("defer", 0), ("in_place", api.RDH_PT_NO_DEFER), ("one_lane", api.RDH_PT_ONE_LANE_PER_PIXEL)):
        gb = api.GBuffer()
        gb.create(w, h)
        got[name] = render(cam, gb, flags | api.RDH_PT_COUNT)
    ref_planes, ref_ct = got["one_lane"]
    full[cname] = {"pixels": w * h, "literal": T.count_literal_primary_rays(cam), "covered": float((ref_planes[3] >= 0).mean()),
                   "one_lane": ref_ct}
    for name in ("defer", "in_place"):
        planes, ct = got[name]
        full[cname][name] = {"counters": ct, "differing": {p: int((a.view(np.uint32) != b.view(np.uint32)).sum())
                                                           for p, a, b in zip(T.PLANES, planes, ref_planes)}}
ctx.close()
with open(f"{out}/results.json", "w") as f:
    json.dump({"counters": counters, "full": full}, f)
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("gbuffer_pairs")
    env = dict(os.environ, RADISH_GBUFFER_PAIRS="1")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), ROOT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, f"child: exit {r.returncode}\n{r.stderr[-3000:]}"  # nothing further is started after a failure
    with open(out / "results.json") as f:
        return out, json.load(f)


def _against_oracle(child, names):
    from oracle import pyoracle

    out, results = child
    cases = _oracle_cases()
    oracles = {}
    for name in names:
        scene, cams, _, count = cases[name]
        if scene not in oracles:
            oracles[scene] = pyoracle.OracleScene(_small_teapots() if scene == "teapots" else chain_scene(1500))
        o = oracles[scene]
        w, h = int(cams[0]["resolution"][0]), int(cams[0]["resolution"][1])
        gb_ref = pyoracle.GBufferHost(w, h)
        for f, cam in enumerate(cams):
            before = o.stats()
            o.gbuffer_render(cam, gb_ref)
            after = o.stats()
            cur = gb_ref.frameIdx
            got = np.load(out / f"{name}_{f}.npz")
            what = f"{name} frame {f}"
            assert np.array_equal(got["primId"], gb_ref.primId[cur]), what
            assert np.array_equal(got["motion"], gb_ref.motion), what
            assert_bit_equal(got["albedo"], gb_ref.albedo, f"{what}: albedo")
            assert_bit_equal(got["normal"], gb_ref.normal[cur], f"{what}: normal")
            assert_bit_equal(got["depth"], gb_ref.depth[cur], f"{what}: depth")
            if count:
                ct = results["counters"][f"{name}_{f}"]
                for k in COUNTERS:
                    assert ct[k] == after[k] - before[k], (what, k)
            gb_ref.update(cam)
        assert (gb_ref.primId[gb_ref.frameIdx ^ 1] >= 0).mean() > 0.2, name


def test_small_teapots_equal_the_oracle(child):
    assert 50 <= count_literal_primary_rays(_cam_axis()) <= 256  # few enough to be set aside
    _against_oracle(child, ["teapots_count", "teapots_plain", "axis_defer", "axis_in_place"])


def test_chain_shaped_tree_equals_the_oracle(child):
    _against_oracle(child, ["chain_count", "chain_plain"])


def test_full_frame_equals_one_lane_per_pixel(child):
    full = child[1]["full"]
    assert full["axis"]["literal"] > 256  # above the cap: none is set aside
    for cname in ("bench", "axis"):
        r = full[cname]
        assert r["one_lane"]["closestRays"] == r["pixels"] and r["covered"] > 0.3, cname
        for name in ("defer", "in_place"):
            assert r[name]["differing"] == {p: 0 for p in PLANES}, (cname, name)
            assert r[name]["counters"] == r["one_lane"], (cname, name)
