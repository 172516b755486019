"""The wavefront path state renumbered every bounce (kernels_wave.h, WaveWorkspace): shade(k) writes what rides with a surviving
path into a fresh slot of the other of two state sets, the accumulators stay at the path's home slot, and home rides in thr.w and
nee.w.

Nothing of that may show: every case compares images bit for bit and the RDH_PT_COUNT counters for equality, against the CPU oracle
on the whole frame.  Depth 8 uses each set four times after raygen's; on the Cornell frame paths die in every bounce (the open front,
the lamp, the depth bound), and at 52x36 (7x5 blocks, partial on both edges) bounce 0's queue holds off-frame -1 entries.
"""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
W, H, DEPTH, LOOPER = 52, 36, 8, 7
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


def _oracle_frame(sd, cam, depth, looper=LOOPER, samples=1):
    """`samples` oracle frames folded into one pair of images (iter 0.., looper, looper + 1, ..), and their summed counters."""
    w, h = (int(v) for v in cam["resolution"])
    d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    stats = {k: 0 for k in COUNTER_KEYS}
    for s in range(samples):
        _, st = oracle_path_trace_mt(sd, cam, d, i, s, looper + s, depth)
        for k in COUNTER_KEYS:
            stats[k] += st[k]
    d.setflags(write=False)
    i.setflags(write=False)
    return {"cam": cam, "d": d, "i": i, "stats": stats}


def _frame(ctx, cam, depth, flags, looper=LOOPER):
    """One frame on the context as it stands (scene and partition are the caller's)."""
    w, h = (int(v) for v in cam["resolution"])
    torch = _torch()
    ctx.set_camera(cam)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace(d, i, 0, looper, depth, flags)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters()


def _render(ctx, sd, cam, depth, flags, looper=LOOPER):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    return _frame(ctx, cam, depth, flags, looper)


def _check(got, ref, what):
    d, i, ct = got
    assert_bit_equal(d, ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(i, ref["i"], f"{what}: indirect vs oracle")
    for k in COUNTER_KEYS:
        assert ct[k] == ref["stats"][k], (what, k, ct[k], ref["stats"][k])


@pytest.fixture(scope="module")
def ref_depth8(cornell_small):
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(W, H)
    ref = _oracle_frame(cornell_small, cam, DEPTH)
    assert ref["d"].max() > 0 and ref["i"].max() > 0 and ref["stats"]["anyRays"] > 0
    # paths die in every bounce and some live to the last: the extension rays of stage k are the difference of two depths' counts
    rays = []
    for depth in range(DEPTH + 1):
        d, i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
        rays.append(oracle_path_trace_mt(cornell_small, cam, d, i, 0, LOOPER, depth)[1]["closestRays"] - sum(rays))
    assert rays[0] == W * H and rays[-1] > 0 and all(a > b for a, b in zip(rays, rays[1:])), rays
    return ref


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("flag_set", FLAG_SETS)
def test_depth_eight_equals_the_oracle(gpu_ctx, cornell_small, ref_depth8, flag_set, walk):
    from radish_pt_amd import api

    _check(_render(gpu_ctx, cornell_small, ref_depth8["cam"], DEPTH, _flags(api, flag_set, walk)), ref_depth8, f"{flag_set}, {walk}")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("flag_set", FLAG_SETS)
def test_first_lists_and_their_overflow_carry_the_new_slots(gpu_ctx, cornell_small, ref_depth8, flag_set, walk):
    from radish_pt_amd import api

    _check(_render(gpu_ctx, cornell_small, ref_depth8["cam"], DEPTH, _flags(api, flag_set, walk, small_lists=True)), ref_depth8,
           f"{flag_set}, {walk}, small lists")


@pytest.mark.parametrize("walk", WALKS)
def test_a_shallow_frame_after_a_deep_one(gpu_ctx, cornell_small, ref_depth8, walk):
    """Depth 8, then depth 2 at another looper on the same context: the deeper frame's state lies stale in both sets."""
    from radish_pt_amd import api

    flags = _flags(api, "wavefront_sort", walk)
    cam = ref_depth8["cam"]
    ref2 = _oracle_frame(cornell_small, cam, 2, looper=31)
    gpu_ctx.set_partition(0, 1, 64)
    gpu_ctx.upload_scene(cornell_small)
    _check(_frame(gpu_ctx, cam, DEPTH, flags), ref_depth8, f"{walk}: depth 8")
    _check(_frame(gpu_ctx, cam, 2, flags, looper=31), ref2, f"{walk}: depth 2 after depth 8")


def test_workspace_regrows_and_is_reused(cornell_small, ref_depth8):
    """52x36, 256x192, 52x36 on one context of its own: the second frame regrows the workspace, the third runs in the big one."""
    from radish_pt_amd import api, scenes

    flags = _flags(api, "wavefront_sort", "pairs")
    big = _oracle_frame(cornell_small, scenes.cornell_camera(256, 192), 3)
    ctx = api.Context(0)
    try:
        ctx.upload_scene(cornell_small)
        _check(_frame(ctx, ref_depth8["cam"], DEPTH, flags), ref_depth8, "first small frame")
        _check(_frame(ctx, big["cam"], 3, flags), big, "256x192")
        _check(_frame(ctx, ref_depth8["cam"], DEPTH, flags), ref_depth8, "small frame in the regrown workspace")
    finally:
        ctx.close()


@pytest.mark.parametrize("flag_set", ("wavefront", "wavefront_sort"))
def test_three_samples_in_one_pass(gpu_ctx, cornell_small, flag_set):
    """path_trace_samples: a sample's home slot is not its pixel index, and k_wf_finish folds a pixel's samples by home."""
    from radish_pt_amd import api, scenes

    samples, depth, looper0 = 3, 4, 11
    ref = _oracle_frame(cornell_small, scenes.cornell_camera(W, H), depth, looper=looper0, samples=samples)
    torch = _torch()
    gpu_ctx.set_partition(0, 1, 64)
    gpu_ctx.upload_scene(cornell_small)
    gpu_ctx.set_camera(ref["cam"])
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    gpu_ctx.counters_reset()
    gpu_ctx.path_trace_samples(d, i, 0, looper0, samples, depth, _flags(api, flag_set, "pairs"), samples_per_pass=samples)
    _check((d.cpu().numpy(), i.cpu().numpy(), gpu_ctx.counters()), ref, f"{flag_set}: three samples")


def test_one_rank_of_a_two_rank_partition(gpu_ctx, cornell_small):
    """160x120 in 64-pixel tiles (3x2, the right and lower ones partial): rank 1's packed tiles equal the oracle's pixels, and the two
    ranks together trace the oracle frame's rays."""
    from radish_pt_amd import api, partition, scenes

    w, h, depth, tile = 160, 120, 4, 64
    ref = _oracle_frame(cornell_small, scenes.cornell_camera(w, h), depth)
    flags = _flags(api, "wavefront_sort", "pairs")
    torch = _torch()
    gpu_ctx.upload_scene(cornell_small)
    gpu_ctx.set_camera(ref["cam"])
    total = {k: 0 for k in COUNTER_KEYS}
    try:
        for rank in (0, 1):
            gpu_ctx.set_partition(rank, 2, tile)
            n = gpu_ctx.tiles_per_rank() * tile * tile
            d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
            gpu_ctx.counters_reset()
            gpu_ctx.path_trace(d, i, 0, LOOPER, depth, flags)
            ct = gpu_ctx.counters()
            for k in COUNTER_KEYS:
                total[k] += ct[k]
            frame_idx, packed_idx = partition.rank_pixels(w, h, rank, 2, tile)
            assert_bit_equal(d.cpu().numpy()[packed_idx], ref["d"][frame_idx], f"rank {rank}: direct vs oracle")
            assert_bit_equal(i.cpu().numpy()[packed_idx], ref["i"][frame_idx], f"rank {rank}: indirect vs oracle")
    finally:
        gpu_ctx.set_partition(0, 1, 64)
    assert total == ref["stats"], (total, ref["stats"])


@pytest.mark.parametrize("walk", WALKS)
def test_unlit_scene_carries_home_through_thr_only(gpu_ctx, cornell_small, walk):
    """The lamp turned into a white wall: no shadow rays, nee is never written, and with an environment map the misses of k > 0 add to
    the home slot they found in thr."""
    from radish_pt_amd import api, layouts as L, scenes

    mats = cornell_small.materials.copy()
    for m in range(len(mats)):
        if mats[m]["type"] == L.LIGHT:
            mats[m] = L.make_material(L.LAMBERTIAN, (0.73, 0.73, 0.73))
    sd = scenes.SceneData("cornell_unlit", cornell_small.vertices, cornell_small.normals, cornell_small.texcoords,
                          cornell_small.material_ids, mats)
    assert sd.num_lights == 0 and len(sd.light_sampler) == 0
    ref = _oracle_frame(sd, scenes.cornell_camera(W, H), DEPTH)
    assert ref["stats"]["anyRays"] == 0 and ref["stats"]["closestRays"] > W * H
    _check(_render(gpu_ctx, sd, ref["cam"], DEPTH, _flags(api, "wavefront_sort", walk)), ref, f"no lights, {walk}")


@pytest.mark.parametrize("walk", WALKS)
def test_textured_scene_with_environment_map(gpu_ctx, walk):
    """The miss branch's addIndirect at k > 0 (environment-map MIS), at depth 8."""
    from radish_pt_amd import api, scenes

    sd = scenes.cornell_textured()
    ref = _oracle_frame(sd, scenes.cornell_camera(40, 24), DEPTH, looper=60)
    assert ref["d"][0].max() > 0 and ref["i"].max() > 0  # the corner pixel sees the environment map
    _check(_render(gpu_ctx, sd, ref["cam"], DEPTH, _flags(api, "wavefront_sort", walk), looper=60), ref, f"textured, {walk}")
