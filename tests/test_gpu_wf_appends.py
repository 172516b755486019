"""The queue appends of the wavefront shade stage (k_wf_shade): one append per packet, the entries staged in the wave's LDS row.

A wave leaves three bits per record in the row it binned its packet into and appends the packet's rays and shadow rays together, so
what can go wrong depends on the packet: 256 records when unsorted, 256 .. 1 024 (multiples of 256) when sorted, as large as leaves
every wave two packets, and the last packet of a stage is cut short.  The small frames of the other wavefront tests only ever see
packets of 256.  Here a 515x403 frame (neither a multiple of 8) is shaded by a 64th of the resident grid: a persistent grid is
capped at 2 048 workgroups of 4 waves, so the share has at most 128 waves, and a stage of more than 2 * 128 * 768 = 196 608
records is binned in packets of 1 024 whatever the resident grid is.  A 16th of the grid bins the same stages in smaller packets
(768, 512 and 256 records with the 768 workgroups that k_wf_shade's three waves per SIMD keep resident on 256 compute units, where
the 64th bins 1 024 throughout), and the full grid in packets of 256.  Every case compares images bit for bit and the
RDH_PT_COUNT counters for equality with the CPU oracle on the whole frame, and what each stage queued (rdh_debug_wf_counts) with
the full grid's.
"""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
W, H, DEPTH, LOOPER = 515, 403, 3, 7
BIG_PACKET_MIN = 2 * (2048 // 64) * 4 * 768  # records of a stage above which a share of 64 bins packets of 1 024


def _flags(api, sort=True, count=True, walk="pairs", small_lists=False):
    f = api.RDH_PT_WAVEFRONT | (api.RDH_PT_SORT_MATERIAL if sort else 0) | (api.RDH_PT_COUNT if count else 0)
    f |= {"pairs": api.RDH_PT_PAIRS, "threaded": api.RDH_PT_NO_PAIRS}[walk]
    return f | (api.RDH_PT_WF_SMALL_LISTS if small_lists else 0)


def _render(ctx, sd, cam, depth, flags, share=1, looper=LOOPER):
    import torch

    w, h = (int(v) for v in cam["resolution"])
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    ctx.counters_reset()
    try:
        ctx.set_occupancy_share(share)
        ctx.path_trace(d, i, 0, looper, depth, flags)
        ctx.synchronize()
        rays, shadows = ctx.debug_wf_counts()
    finally:
        ctx.set_occupancy_share(1)
    return d.cpu().numpy(), i.cpu().numpy(), ctx.counters(), rays, shadows


def _check(got, ref, what, counters=True):
    assert_bit_equal(got[0], ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(got[1], ref["i"], f"{what}: indirect vs oracle")
    if counters:
        for k in COUNTER_KEYS:
            assert got[2][k] == ref["stats"][k], (what, k, got[2][k], ref["stats"][k])


@pytest.fixture(scope="module")
def ref(cornell_small):
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(W, H)
    d, i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    _, st = oracle_path_trace_mt(cornell_small, cam, d, i, 0, LOOPER, DEPTH)
    d.setflags(write=False)
    i.setflags(write=False)
    assert d.max() > 0 and i.max() > 0 and st["anyRays"] > 0
    return {"cam": cam, "d": d, "i": i, "stats": {k: st[k] for k in COUNTER_KEYS}}


@pytest.fixture(scope="module")
def full_grid(gpu_ctx, cornell_small, ref):
    """The sorted, counted frame on the whole resident grid: what every stage queued, for the other schedules to equal."""
    from radish_pt_amd import api

    got = _render(gpu_ctx, cornell_small, ref["cam"], DEPTH, _flags(api))
    _check(got, ref, "full grid")
    rays, shadows = got[3], got[4]
    assert len(rays) == DEPTH + 1 and rays[0] >= ((W + 7) // 8) * ((H + 7) // 8) * 64  # (whole ownership tiles)
    assert rays[0] > BIG_PACKET_MIN and all(0 < rays[k + 1] < rays[k] for k in range(DEPTH)), rays
    assert all(s > 0 for s in shadows[:DEPTH]), shadows
    return rays, shadows


@pytest.mark.parametrize("walk", ("pairs", "threaded"))
@pytest.mark.parametrize("sort", (True, False))
@pytest.mark.parametrize("share", (64, 16))
def test_share_of_the_grid_bins_large_packets(gpu_ctx, cornell_small, ref, full_grid, share, sort, walk):
    from radish_pt_amd import api

    got = _render(gpu_ctx, cornell_small, ref["cam"], DEPTH, _flags(api, sort=sort, walk=walk), share=share)
    _check(got, ref, f"share {share}, sort {sort}, {walk}")
    assert np.array_equal(got[3], full_grid[0]) and np.array_equal(got[4], full_grid[1]), (got[3], got[4], full_grid)


def test_default_frame_skips_rays_and_keeps_the_image(gpu_ctx, cornell_small, ref, full_grid):
    """Without RDH_PT_COUNT the stage queues fewer rays (the rays whose outcome cannot reach the image): other counts, same image."""
    from radish_pt_amd import api

    got = _render(gpu_ctx, cornell_small, ref["cam"], DEPTH, _flags(api, count=False), share=64)
    _check(got, ref, "share 64, default frame", counters=False)
    assert got[3][0] == full_grid[0][0] and got[4].sum() <= full_grid[1].sum(), (got[3], got[4], full_grid)


def test_small_lists_mark_their_entries_in_the_ray_queue(gpu_ctx, cornell_small, ref, full_grid):
    """Lists of four entries: a listed extension ray's queue entry is -2 - slot (the third staged bit), a listed shadow ray has
    none, and what does not fit the list stays in the queues."""
    from radish_pt_amd import api

    got = _render(gpu_ctx, cornell_small, ref["cam"], DEPTH, _flags(api, small_lists=True), share=64)
    _check(got, ref, "share 64, small lists")
    assert np.array_equal(got[3], full_grid[0]) and np.array_equal(got[4], full_grid[1]), (got[3], got[4], full_grid)


@pytest.mark.parametrize("depth", (0, 1))
def test_shallow_frames(gpu_ctx, cornell_small, depth):
    """Depth 0: shade(0) is the last stage and appends nothing that is traced; depth 1: its appends are the frame's only ones."""
    from radish_pt_amd import api, scenes

    cam = scenes.cornell_camera(W, H)
    d, i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    _, st = oracle_path_trace_mt(cornell_small, cam, d, i, 0, LOOPER, depth)
    r = {"d": d, "i": i, "stats": {k: st[k] for k in COUNTER_KEYS}}
    _check(_render(gpu_ctx, cornell_small, cam, depth, _flags(api), share=64), r, f"depth {depth}")


def test_three_samples_in_one_pass(gpu_ctx, cornell_small):
    """Three samples of a 300x230 frame in one pass: 3 * 38 * 29 * 64 = 211 584 records in stage 0, above the bound again; the
    images equal three single passes on the full grid (which tests/test_gpu_samples.py holds to the oracle)."""
    import torch

    from radish_pt_amd import api, scenes

    w, h = 300, 230
    assert 3 * ((w + 7) // 8) * ((h + 7) // 8) * 64 > BIG_PACKET_MIN
    cam = scenes.cornell_camera(w, h)
    flags = _flags(api, count=False)
    gpu_ctx.set_partition(0, 1, 64)
    gpu_ctx.upload_scene(cornell_small)
    gpu_ctx.set_camera(cam)
    one_d, one_i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    for s in range(3):
        gpu_ctx.path_trace(one_d, one_i, s, LOOPER + s, DEPTH, flags)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    try:
        gpu_ctx.set_occupancy_share(64)
        gpu_ctx.path_trace_samples(d, i, 0, LOOPER, 3, DEPTH, flags, samples_per_pass=3)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_occupancy_share(1)
    assert one_d.max() > 0
    assert_bit_equal(d.cpu().numpy(), one_d.cpu().numpy(), "three samples in one pass: direct")
    assert_bit_equal(i.cpu().numpy(), one_i.cpu().numpy(), "three samples in one pass: indirect")
