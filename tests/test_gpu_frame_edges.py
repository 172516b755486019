"""The frame kernels at the ends of their two axes (inputs: tests/frame_edges.py, held to their conditions by
tests/test_frame_edges_cpu.py): frames from one pixel to one over the 64-pixel tile, paths of 28 bounces — the most rdh_path_trace
accepts — in a closed room where nine paths in ten live that long, the last word of the Sobol table, and ranks of a tile partition
that own no pixel.

Everything is compared with the CPU oracle bit for bit; with RDH_PT_COUNT the five work counters are compared for equality as well.
Without that flag the wavefront structures skip the bounce-28 rays that cannot reach the image (RD_WF_CULL_LAST, now at k = 27); with
it they walk every ray.
"""
import numpy as np
import pytest

import frame_edges as FE
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

SHAPES = list(FE.SHAPES)
IDS = [FE.SHAPE_IDS[s] for s in SHAPES]
STRUCTURES = ("mega", "persistent", "persistent_threaded", "wavefront", "wavefront_sort", "wavefront_threaded")
COUNT = pytest.mark.parametrize("count", [True, False], ids=["count", "nocount"])
DEPTH = FE.MAX_DEPTH


def _torch():
    import torch

    return torch


def _flags(api, structure, count):
    f = {"mega": api.RDH_PT_MEGAKERNEL, "persistent": api.RDH_PT_PERSISTENT,
         "persistent_threaded": api.RDH_PT_PERSISTENT | api.RDH_PT_NO_PAIRS,
         "wavefront": api.RDH_PT_WAVEFRONT, "wavefront_sort": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL,
         "wavefront_threaded": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_NO_PAIRS}[structure]
    return f | (api.RDH_PT_COUNT if count else 0)


def _own_context(sd):
    from radish_pt_amd import api

    ctx = api.Context(0)
    ctx.upload_scene(sd)
    return ctx


@pytest.fixture(scope="module")
def closed_ctx(gpu_ctx):
    """The closed room, uploaded once for the module (on a context of the module's own: gpu_ctx is every module's)."""
    ctx = _own_context(FE.closed_scene())
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def glass_free_ctx(gpu_ctx):
    ctx = _own_context(FE.closed_scene(False))
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def teapots_ctx(gpu_ctx):
    ctx = _own_context(FE.teapots_scene())
    yield ctx
    ctx.close()


def _frames(ctx, cam, depth, flags, looper, frames=1):
    """`frames` accumulated frames (iter 0.., consecutive loopers) on the context as it stands."""
    w, h = (int(v) for v in cam["resolution"])
    torch = _torch()
    ctx.set_camera(cam)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    ctx.counters_reset()
    for f in range(frames):
        ctx.path_trace(d, i, f, (looper + f) % 10000, depth, flags)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters()


def _check(got, ref, what, count):
    d, i, ct = got
    assert_bit_equal(d, ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(i, ref["i"], f"{what}: indirect vs oracle")
    if count:
        for k in FE.COUNTER_KEYS:
            assert ct[k] == ref["stats"][k], (what, k, ct[k], ref["stats"][k])


# ---------------------------------------------------------------------------------------------------------------------------------
# path tracer, depth 28
# ---------------------------------------------------------------------------------------------------------------------------------
@COUNT
@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_depth_28_at_every_shape(closed_ctx, shape, structure, count):
    """Two accumulated frames (iter 0 and 1, consecutive loopers) of the closed room."""
    from radish_pt_amd import api

    looper = FE.closed_looper(shape)
    ref = FE.closed_ref(shape, DEPTH, looper, 2)
    _check(_frames(closed_ctx, ref["cam"], DEPTH, _flags(api, structure, count), looper, 2), ref,
           f"{FE.SHAPE_IDS[shape]} {structure}", count)


@COUNT
def test_small_literal_lists_overflow_at_late_stages(closed_ctx, count):
    from radish_pt_amd import api

    looper = FE.closed_looper(FE.BASE)
    ref = FE.closed_ref(FE.BASE, DEPTH, looper, 2)
    flags = _flags(api, "wavefront_sort", count) | api.RDH_PT_WF_SMALL_LISTS
    _check(_frames(closed_ctx, ref["cam"], DEPTH, flags, looper, 2), ref, "small lists", count)


@pytest.mark.parametrize("structure", ("wavefront_sort", "persistent"))
@pytest.mark.parametrize("depth", (9, 16, 27, 28))
def test_depth_sweep_pins_the_stage_count(closed_ctx, depth, structure):
    from radish_pt_amd import api

    looper = FE.closed_looper(FE.BASE)
    ref = FE.closed_ref(FE.BASE, depth, looper, 1)
    _check(_frames(closed_ctx, ref["cam"], depth, _flags(api, structure, True), looper), ref, f"depth {depth} {structure}", True)


@pytest.mark.parametrize("structure", ("wavefront", "wavefront_sort"))
@pytest.mark.parametrize("shape", [(16, 8), FE.BASE, (16, 16)], ids=["16x8", "16x12", "16x16"])
def test_every_stage_queues_the_oracles_rays(closed_ctx, shape, structure):
    """What trace(k) finds in its ray queue, k = 1..28, is what the oracle traces at bounce k (rdh_debug_wf_counts against the
    difference of two depths' closest-hit counts): the queues stay nine tenths full to the last stage.  A counting frame walks every
    ray; a default frame queues the same rays in every stage but the last, where it drops those that cannot reach the lamp."""
    from radish_pt_amd import api

    looper = FE.closed_looper(shape)
    want = FE.bounce_rays(shape, looper)
    ref = FE.closed_ref(shape, DEPTH, looper, 1)
    queued = {}
    for count in (True, False):
        _check(_frames(closed_ctx, ref["cam"], DEPTH, _flags(api, structure, count), looper), ref, f"{FE.SHAPE_IDS[shape]} {structure}", count)
        rays, _ = closed_ctx.debug_wf_counts()
        assert len(rays) == DEPTH + 1
        queued[count] = [int(v) for v in rays]
    assert queued[True][0] == queued[False][0] == 64 * 64  # bounce 0's queue is the identity over one 64-pixel tile's 64 blocks
    assert queued[True][1:] == list(want[1:]), (queued[True], want)
    assert queued[False][1:DEPTH] == list(want[1:DEPTH])
    assert queued[False][DEPTH] < want[DEPTH], (queued[False][DEPTH], want[DEPTH])
    assert want[DEPTH] * 2 >= shape[0] * shape[1]


@COUNT
@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("shape", [FE.BASE, (1, 1)], ids=["16x12", "1x1"])
def test_last_word_of_the_sobol_table(glass_free_ctx, shape, structure, count):
    """looper 9999 without a dielectric: the 200th value of a path alive at bounce 28 is table[9999][199], and the half-metallic
    wall's lobe choice depends on it (test_frame_edges_cpu.py)."""
    from radish_pt_amd import api

    ref = FE.closed_ref(shape, DEPTH, FE.LAST_ROW, 1, False)
    _check(_frames(glass_free_ctx, ref["cam"], DEPTH, _flags(api, structure, count), FE.LAST_ROW), ref,
           f"last word {FE.SHAPE_IDS[shape]} {structure}", count)


# ---------------------------------------------------------------------------------------------------------------------------------
# several samples in one call
# ---------------------------------------------------------------------------------------------------------------------------------
def _samples(ctx, ref, looper, samples, flags, samples_per_pass):
    w, h = (int(v) for v in ref["cam"]["resolution"])
    torch = _torch()
    ctx.set_camera(ref["cam"])
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    ctx.counters_reset()
    ctx.path_trace_samples(d, i, 0, looper, samples, DEPTH, flags, samples_per_pass=samples_per_pass)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters()


@COUNT
@pytest.mark.parametrize("samples_per_pass", (4, 1))
@pytest.mark.parametrize("structure", ("wavefront", "wavefront_sort"))
@pytest.mark.parametrize("shape", [(7, 9), FE.BASE], ids=["7x9", "16x12"])
def test_four_samples_across_the_looper_wrap(closed_ctx, shape, structure, samples_per_pass, count):
    """Rows 9998, 9999, 0, 1 at depth 28, in one pass and in four."""
    from radish_pt_amd import api

    ref = FE.closed_ref(shape, DEPTH, 9998, 4)
    got = _samples(closed_ctx, ref, 9998, 4, _flags(api, structure, count), samples_per_pass)
    _check(got, ref, f"{FE.SHAPE_IDS[shape]} {structure} samples_per_pass={samples_per_pass}", count)


@COUNT
@pytest.mark.parametrize("shape", [(1, 1), (8, 8)], ids=["1x1", "8x8"])
def test_sixteen_samples_in_one_pass(closed_ctx, shape, count):
    """One pixel in 16 slots (1x1), one full block 16 times (8x8): 1024 slots either way."""
    from radish_pt_amd import api

    looper = FE.closed_looper(shape)
    ref = FE.closed_ref(shape, DEPTH, looper, 16)
    got = _samples(closed_ctx, ref, looper, 16, _flags(api, "wavefront_sort", count), 16)
    _check(got, ref, f"{FE.SHAPE_IDS[shape]} 16 samples", count)


# ---------------------------------------------------------------------------------------------------------------------------------
# frame order on one context
# ---------------------------------------------------------------------------------------------------------------------------------
@COUNT
def test_tiny_frame_after_a_large_deep_one(count):
    """63x65 at depth 28, 1x1 at depth 28, 16x12 at depth 2, 63x65 again: the stale state of a larger, deeper frame lies in both
    state sets under a tiny one."""
    from radish_pt_amd import api

    flags = _flags(api, "wavefront_sort", count)
    order = [((63, 65), DEPTH), ((1, 1), DEPTH), (FE.BASE, 2), ((63, 65), DEPTH)]
    ctx = _own_context(FE.closed_scene())
    try:
        for n, (shape, depth) in enumerate(order):
            looper = FE.closed_looper(shape)
            ref = FE.closed_ref(shape, depth, looper, 1)
            _check(_frames(ctx, ref["cam"], depth, flags, looper), ref, f"frame {n}: {FE.SHAPE_IDS[shape]} depth {depth}", count)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# ranks with nothing to do
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", ("persistent", "wavefront_sort"))
@pytest.mark.parametrize("part", FE.PARTITIONS, ids=[f"{FE.SHAPE_IDS[s]}-tile{t}-world{w}" for s, t, w in FE.PARTITIONS])
def test_ranks_whose_share_is_empty(closed_ctx, part, structure):
    from radish_pt_amd import api, partition

    shape, tile, world = part
    w, h = shape
    looper = FE.closed_looper(shape)
    ref = FE.closed_ref(shape, DEPTH, looper, 1)
    flags = _flags(api, structure, True)
    torch = _torch()
    closed_ctx.set_camera(ref["cam"])
    total = {k: 0 for k in FE.COUNTER_KEYS}
    empty_ranks = 0
    try:
        for rank in range(world):
            closed_ctx.set_partition(rank, world, tile)
            n = closed_ctx.tiles_per_rank() * tile * tile
            assert n == partition.shard_elems(w, h, world, tile)
            pattern = (torch.arange(3 * n, device="cuda", dtype=torch.float32).reshape(n, 3) % 251.0) + 0.5
            d, i = pattern.clone(), pattern.clone() + 1000.0
            before = (d.cpu().numpy().tobytes(), i.cpu().numpy().tobytes())
            closed_ctx.counters_reset()
            closed_ctx.path_trace(d, i, 0, looper, DEPTH, flags)  # raises unless RDH_OK
            ct = closed_ctx.counters()
            got_d, got_i = d.cpu().numpy(), i.cpu().numpy()
            frame_idx, packed_idx = partition.rank_pixels(w, h, rank, world, tile)
            assert_bit_equal(got_d[packed_idx], ref["d"][frame_idx], f"rank {rank}: direct vs oracle")
            assert_bit_equal(got_i[packed_idx], ref["i"][frame_idx], f"rank {rank}: indirect vs oracle")
            for k in FE.COUNTER_KEYS:
                total[k] += ct[k]
            if len(frame_idx) == 0:
                empty_ranks += 1
                assert all(ct[k] == 0 for k in FE.COUNTER_KEYS), (rank, ct)
                assert (got_d.tobytes(), got_i.tobytes()) == before, f"rank {rank} owns no pixel and wrote to its buffers"
    finally:
        closed_ctx.set_partition(0, 1, 64)
    assert total == ref["stats"], (total, ref["stats"])
    num_tiles = ((w + tile - 1) // tile) * ((h + tile - 1) // tile)
    assert (empty_ranks >= 1) == (world > num_tiles)


# ---------------------------------------------------------------------------------------------------------------------------------
# direct lighting
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_direct_lighting_at_every_shape(closed_ctx, shape):
    ref = FE.direct_ref(shape)
    w, h = shape
    closed_ctx.set_camera(ref["cam"])
    d = _torch().zeros(w * h, 3, device="cuda")
    for it in range(ref["iters"]):
        closed_ctx.path_trace_direct(d, it, ref["looper0"] + it)
    assert_bit_equal(d.cpu().numpy(), ref["d"], f"{FE.SHAPE_IDS[shape]}: pathTraceDirect")
    assert ref["d"].max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# G-buffer and ReSTIR
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_planes(gb, want, what):
    cur = gb.frameIdx
    assert np.array_equal(gb.primId[cur].cpu().numpy(), want["primId"]), f"{what}: primId"
    assert np.array_equal(gb.motion.cpu().numpy(), want["motion"]), f"{what}: motion"
    assert_bit_equal(gb.albedo.cpu().numpy(), want["albedo"], f"{what}: albedo")
    assert_bit_equal(gb.normal[cur].cpu().numpy(), want["normal"], f"{what}: normal")
    assert_bit_equal(gb.depth[cur].cpu().numpy(), want["depth"], f"{what}: depth")


@pytest.mark.parametrize("kernel", ["packets", "packets_budget_4", "persistent", "one_lane_per_pixel"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gbuffer_kernels_at_every_shape(teapots_ctx, shape, kernel):
    from radish_pt_amd import api

    w, h = shape
    flags = api.RDH_PT_COUNT | {"one_lane_per_pixel": api.RDH_PT_MEGA_GBUFFER, "persistent": api.RDH_PT_NO_PACKETS, "packets": 0,
                                "packets_budget_4": api.RDH_PT_WF_SMALL_LISTS}[kernel]
    gb = api.GBuffer()
    gb.create(w, h)
    for f, frame in enumerate(FE.gbuffer_ref(shape)):
        cam = frame["cam"]
        teapots_ctx.set_camera(cam)
        teapots_ctx.counters_reset()
        teapots_ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), flags)
        teapots_ctx.synchronize()
        _check_planes(gb, frame["planes"], f"{FE.SHAPE_IDS[shape]} {kernel} frame {f}")
        ct = teapots_ctx.counters()
        for k in ("closestRays", "nodeVisits", "triTests", "closestHits"):
            assert ct[k] == frame["stats"][k], (k, ct[k], frame["stats"][k])
        gb.update(cam)


@pytest.mark.parametrize("faithful", [1, 0])
@pytest.mark.parametrize("reuse", [0, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restir_sequence_at_every_shape(teapots_ctx, shape, reuse, faithful):
    """The three-frame moving-camera sequence; spatial reuse searches a disk of radius 5 around a pixel, which reaches past the frame
    from every pixel of seven of the shapes."""
    from radish_pt_amd import api

    w, h = shape
    ctx = teapots_ctx
    ref = FE.restir_ref(shape, reuse, faithful)
    gb = api.GBuffer()
    gb.create(w, h)
    img = _torch().zeros(w * h, 3, device="cuda")
    ctx.set_camera(ref[0]["cam"])
    ctx.restir_init()
    try:
        for f, frame in enumerate(ref):
            cam = frame["cam"]
            ctx.set_camera(cam)
            ctx.gbuffer_render(gb.c_struct(cam_fallback=cam), 0)
            ctx.synchronize()
            assert np.array_equal(gb.primId[gb.frameIdx].cpu().numpy(), frame["primId"]), f"frame {f}: G-buffer ids"
            ctx.counters_reset()
            ctx.restir_direct(img, 0, 40 + f, gb.c_struct(cam), reuse, faithful_ris=faithful,
                              flags=api.RDH_PT_COUNT | (0 if faithful else api.RDH_PT_NO_PACKETS)
                              | (api.RDH_PT_WF_SMALL_LISTS if (faithful and reuse == 3) else 0))  # as test_restir_sequence_bit_exact
            what = f"{FE.SHAPE_IDS[shape]} reuse={reuse} faithful={faithful} frame {f}"
            assert_bit_equal(img.cpu().numpy(), frame["img"], f"{what}: image")
            assert ctx.restir_read(1).tobytes() == frame["reservoirs"], f"{what}: reservoirs"
            ct = ctx.counters()
            for k in FE.COUNTER_KEYS:
                assert ct[k] == frame["stats"][k], (what, k, ct[k], frame["stats"][k])
            gb.update(cam)
    finally:
        ctx.restir_free()


# ---------------------------------------------------------------------------------------------------------------------------------
# display
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 65)], ids=["1x1", "1x65"])
def test_copy_image_to_pbo_at_tiny_frames(closed_ctx, shape):
    from oracle import pyoracle

    torch = _torch()
    w, h = shape
    n = w * h
    rng = np.random.default_rng(7)
    img = (rng.random((n, 3)).astype(np.float32) ** 3) * 6.0
    special = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-42, 1.0, 255.0, 1e30], np.float32)[: min(n, 10)]
    img[: len(special), 0] = special
    img[: len(special), 1] = special[::-1]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    pbo = torch.full((n, 4), 77, dtype=torch.uint8, device="cuda")
    for tone in (0, 1, 2):
        for scale in (1.0, 0.37):
            closed_ctx.copy_image_to_pbo(pbo, dev(img), w, h, 0, tone, scale)
            assert np.array_equal(pbo.cpu().numpy(), pyoracle.copy_image_to_pbo(img, w, h, 0, tone, scale)), f"vec3 tone={tone} scale={scale}"
    rg = rng.random((n, 2)).astype(np.float32) * 1.5 - 0.2
    closed_ctx.copy_image_to_pbo(pbo, dev(rg), w, h, 1)
    assert np.array_equal(pbo.cpu().numpy(), pyoracle.copy_image_to_pbo(rg, w, h, 1))
    g = rng.random(n).astype(np.float32) * 3.0
    closed_ctx.copy_image_to_pbo(pbo, dev(g), w, h, 2)
    assert np.array_equal(pbo.cpu().numpy(), pyoracle.copy_image_to_pbo(g, w, h, 2))
    mv = rng.integers(-1, n, n).astype(np.int32)
    closed_ctx.copy_image_to_pbo(pbo, dev(mv), w, h, 3)
    assert np.array_equal(pbo.cpu().numpy(), pyoracle.copy_image_to_pbo(mv, w, h, 3))
