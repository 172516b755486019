"""The item order of a wavefront trace stage (k_wf_trace): extension rays [0, nRay), then shadow rays [nRay, nRay + nShadow).

Nothing may depend on the order: every case compares images bit for bit and the RDH_PT_COUNT counters for equality, against the CPU
oracle on the whole frame.  The frames are small on purpose: at 52x36 every stage's nRay and nShadow are far from multiples of the
128-item packet, so the boundary between the two kinds falls inside a packet; with the literal-class lists cut to four entries
(RDH_PT_WF_SMALL_LISTS) what overflows them stays in the ordinary queues, in both kinds; with a 64th of the grid the shared head hands out what the
static first packets do not cover: shadow rays at 160x120, the end of the extension rays and the boundary packet too at 256x192.
"""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
W, H, DEPTH, LOOPER = 52, 36, 3, 7
FLAG_SETS = ("wavefront", "wavefront_sort", "wavefront_sort_subframes")
WALKS = ("pairs", "threaded")


def _torch():
    import torch

    return torch


def _flags(api, flag_set, walk, small_lists=False):
    f = {"wavefront": api.RDH_PT_WAVEFRONT,
         "wavefront_sort": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL,
         "wavefront_sort_subframes": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES}[flag_set]
    f |= {"pairs": api.RDH_PT_PAIRS, "threaded": api.RDH_PT_NO_PAIRS}[walk]
    if small_lists:
        f |= api.RDH_PT_WF_SMALL_LISTS
    return f | api.RDH_PT_COUNT


def _oracle_frame(sd, cam, depth, looper=LOOPER):
    w, h = (int(v) for v in cam["resolution"])
    d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    _, st = oracle_path_trace_mt(sd, cam, d, i, 0, looper, depth)
    d.setflags(write=False)
    i.setflags(write=False)
    return {"cam": cam, "d": d, "i": i, "stats": {k: st[k] for k in COUNTER_KEYS}}


def _render(ctx, sd, cam, depth, flags, looper=LOOPER):
    w, h = (int(v) for v in cam["resolution"])
    torch = _torch()
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, looper, depth, flags)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters()


def _check(got, ref, what):
    d, i, ct = got
    assert_bit_equal(d, ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(i, ref["i"], f"{what}: indirect vs oracle")
    for k in COUNTER_KEYS:
        assert ct[k] == ref["stats"][k], (what, k, ct[k], ref["stats"][k])


@pytest.fixture(scope="module")
def ref_depth3(cornell_small):
    from radish_pt_amd import scenes

    ref = _oracle_frame(cornell_small, scenes.cornell_camera(W, H), DEPTH)
    assert ref["d"].max() > 0 and ref["i"].max() > 0 and ref["stats"]["anyRays"] > 0
    return ref


@pytest.fixture(scope="module")
def ref_depth1(cornell_small):
    from radish_pt_amd import scenes

    ref = _oracle_frame(cornell_small, scenes.cornell_camera(W, H), 1)
    assert ref["stats"]["anyRays"] > 0  # the shadow rays of trace(1), whose paths end in shade(1)
    return ref


@pytest.fixture(scope="module")
def unlit_scene(cornell_small):
    """The Cornell scene with its lamp turned into a white wall: no emissive triangle, so nShadow = 0 in every stage."""
    from radish_pt_amd import layouts as L, scenes

    mats = cornell_small.materials.copy()
    for m in range(len(mats)):
        if mats[m]["type"] == L.LIGHT:
            mats[m] = L.make_material(L.LAMBERTIAN, (0.73, 0.73, 0.73))
    sd = scenes.SceneData("cornell_unlit", cornell_small.vertices, cornell_small.normals, cornell_small.texcoords,
                          cornell_small.material_ids, mats)
    assert sd.num_lights == 0 and len(sd.light_sampler) == 0
    return sd


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("flag_set", FLAG_SETS)
def test_frame_equals_the_oracle(gpu_ctx, cornell_small, ref_depth3, flag_set, walk):
    from radish_pt_amd import api

    _check(_render(gpu_ctx, cornell_small, ref_depth3["cam"], DEPTH, _flags(api, flag_set, walk)), ref_depth3, f"{flag_set}, {walk}")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("flag_set", FLAG_SETS)
def test_small_lists_overflow_into_the_queues(gpu_ctx, cornell_small, ref_depth3, flag_set, walk):
    from radish_pt_amd import api

    _check(_render(gpu_ctx, cornell_small, ref_depth3["cam"], DEPTH, _flags(api, flag_set, walk, small_lists=True)), ref_depth3,
           f"{flag_set}, {walk}, small lists")


@pytest.mark.parametrize("walk", WALKS)
def test_depth_one_ends_on_shadow_rays(gpu_ctx, cornell_small, ref_depth1, walk):
    from radish_pt_amd import api

    _check(_render(gpu_ctx, cornell_small, ref_depth1["cam"], 1, _flags(api, "wavefront_sort", walk)), ref_depth1, f"depth 1, {walk}")


@pytest.mark.parametrize("walk", WALKS)
def test_scene_without_lights_has_no_shadow_rays(gpu_ctx, unlit_scene, walk):
    from radish_pt_amd import api, scenes

    ref = _oracle_frame(unlit_scene, scenes.cornell_camera(W, H), DEPTH)
    assert ref["stats"]["anyRays"] == 0 and ref["stats"]["closestRays"] > W * H
    _check(_render(gpu_ctx, unlit_scene, ref["cam"], DEPTH, _flags(api, "wavefront_sort", walk)), ref, f"no lights, {walk}")


@pytest.mark.parametrize("walk", WALKS)
def test_textured_scene_with_environment_map(gpu_ctx, walk):
    from radish_pt_amd import api, scenes

    sd = scenes.cornell_textured()
    ref = _oracle_frame(sd, scenes.cornell_camera(40, 24), DEPTH, looper=60)
    assert ref["d"][0].max() > 0  # the corner pixel sees the environment map
    _check(_render(gpu_ctx, sd, ref["cam"], DEPTH, _flags(api, "wavefront_sort", walk), looper=60), ref, f"textured, {walk}")


@pytest.mark.parametrize("w,h,head_reaches_extension_rays", [(160, 120, False), (256, 192, True)])
def test_shared_head_hands_out_across_the_kind_boundary(gpu_ctx, cornell_small, w, h, head_reaches_extension_rays):
    """A 64th of the resident grid, so that the static first packets (128 items per wave of the grid) do not cover stage 1 and the
    shared head hands out the rest: at 160x120 the packet that holds the boundary or the shadow rays behind it, at 256x192 also the
    end of the extension rays (about half of this camera's primary rays leave through the open front, so stage 1 holds ~0.55 w h
    extension rays and as many shadow rays).

    The library does not report its resident grid, so the share is the largest one (64) and the static share is bounded from above:
    a persistent grid is capped at 2 048 workgroups (kPersistentGrid) of 4 waves, and a wave's first packet is 128 items."""
    from radish_pt_amd import api, scenes

    static_share_max = (2048 // 64) * 4 * 128
    cam = scenes.cornell_camera(w, h)
    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT
    ref = _oracle_frame(cornell_small, cam, DEPTH)
    # rays of stage 1 from the counters: a depth-1 frame traces stages 0 and 1, a depth-0 frame stage 0 alone
    c0 = _render(gpu_ctx, cornell_small, cam, 0, flags)[2]
    c1 = _render(gpu_ctx, cornell_small, cam, 1, flags)[2]
    n_ray1, n_shadow1 = c1["closestRays"] - c0["closestRays"], c1["anyRays"] - c0["anyRays"]
    assert c0["anyRays"] == 0 and n_shadow1 > 0
    assert n_ray1 + n_shadow1 > static_share_max, (n_ray1, n_shadow1, static_share_max)
    if head_reaches_extension_rays:
        assert n_ray1 > static_share_max, (n_ray1, static_share_max)
    whole = _render(gpu_ctx, cornell_small, cam, DEPTH, flags)
    try:
        gpu_ctx.set_occupancy_share(64)
        part = _render(gpu_ctx, cornell_small, cam, DEPTH, flags)
    finally:
        gpu_ctx.set_occupancy_share(1)
    assert_bit_equal(part[0], whole[0], "share 64 vs share 1: direct")
    assert_bit_equal(part[1], whole[1], "share 64 vs share 1: indirect")
    assert part[2] == whole[2]
    _check(part, ref, "share 64")
    _check(whole, ref, "share 1")
