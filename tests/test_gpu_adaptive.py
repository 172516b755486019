"""Adaptive sampling on the GPU (rdh_path_trace_adaptive, rdh_adaptive_plan, Context.converge).

Contract: for every pixel with r = request[p] > 0 and c = count[p] the two images are bit for bit those of path_trace at
iter c + j, looper (looper + c + j) % 10000, j = 0..r-1, the count becomes c + r and the moments are folded alike; a pixel without a
request is written in no plane; with RDH_PT_COUNT the counters are those of the requested (pixel, sample) pairs.

Everything expected comes from the CPU oracle (tests/adaptive_oracle.py): whole frames per sample index, gathered per pixel at its
own count, single-pixel calls for the counters, and the numpy model (tests/adaptive_model.py) for the moments and the plan.  The frame
is the 52x36 one of test_gpu_samples.py, looper 9998 so that the rows wrap inside every pixel's sequence, depth 4.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as am
import adaptive_oracle as ao
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu
PLAN_THRESHOLD = am.PLAN_THRESHOLD

W, H, DEPTH, LOOPER = 52, 36, 4, 9998
P = W * H
NUM = 24  # sample indices the oracle renders: counts of 0..7 and requests of up to 16
SENTINEL_F, SENTINEL_C = -7.25, -3  # what an unrequested pixel holds before the call (a count the entry would refuse if it read it)
COUNTER_KEYS = ao.COUNTER_KEYS


def _torch():
    import torch

    return torch


def _flags(api, name):
    wf = api.RDH_PT_WAVEFRONT
    return {"wavefront": wf, "sort": wf | api.RDH_PT_SORT_MATERIAL, "no_pairs": wf | api.RDH_PT_NO_PAIRS,
            "small_lists": wf | api.RDH_PT_WF_SMALL_LISTS, "walk_all": wf | api.RDH_PT_WALK_ALL}[name]


def _use(ctx, sd, cam):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)


def _f(a):
    return _torch().from_numpy(np.array(a, dtype=np.float32, copy=True)).cuda()


def _i(a):
    return _torch().from_numpy(np.array(a, dtype=np.int32, copy=True)).cuda()


@pytest.fixture(scope="module")
def cam():
    from radish_pt_amd import scenes

    return scenes.cornell_camera(W, H)


@pytest.fixture(scope="module")
def ref(cornell_small, cam):
    return ao.frames(cornell_small, cam, LOOPER, NUM, DEPTH)


def _uneven(seed, num_pixels=P, w=W):
    """Requests from a seeded draw in 0..16 with whole blocks at 0 and some blocks holding a single pixel; counts in 0..7."""
    rng = np.random.default_rng(seed)
    request = rng.integers(0, 17, num_pixels).astype(np.int32)
    count = rng.integers(0, 8, num_pixels).astype(np.int32)
    y, x = np.divmod(np.arange(num_pixels), w)
    block = (y // 8) * ((w + 7) // 8) + x // 8
    blocks = rng.permutation(block.max() + 1)
    for b in blocks[:8]:
        request[block == b] = 0
    for b in blocks[8:13]:
        keep = rng.choice(np.flatnonzero(block == b))
        request[(block == b) & (np.arange(num_pixels) != keep)] = 0
        request[keep] = rng.integers(1, 17)
    return count, request


def _plane_with_sum(total, seed):
    rng = np.random.default_rng(seed)
    request = np.zeros(P, np.int32)
    left = total
    for p in rng.permutation(P):
        if left == 0:
            break
        request[p] = min(left, int(rng.integers(1, 17)))
        left -= request[p]
    assert request.sum() == total
    return rng.integers(0, 8, P).astype(np.int32), request


def _run_and_check(ctx, fr, count, request, flags, what, looper=LOOPER, depth=DEPTH, moments=True, counters=None):
    """One call on planes made from the oracle (requested pixels: its means and the model's moments at the pixel's own count;
    the others: sentinels), then every plane against the oracle at count + request."""
    on = request > 0
    d0, i0 = ao.means_at(fr, count)
    m0 = ao.moments_after(fr, count)
    c0 = count.copy()
    d0[~on], i0[~on], m0[~on], c0[~on] = SENTINEL_F, SENTINEL_F, SENTINEL_F, SENTINEL_C
    d, i, c, r = _f(d0), _f(i0), _i(c0), _i(request)
    m = _f(m0) if moments else None
    ctx.counters_reset()
    traced = ctx.path_trace_adaptive(d, i, c, r, looper, depth, flags, moments=m)
    ct = ctx.counters()
    assert traced == int(request.sum()), what
    ed, ei = ao.means_at(fr, count + request)
    em = ao.moments_after(fr, count + request)
    ec = count + request
    ed[~on], ei[~on], em[~on], ec[~on] = SENTINEL_F, SENTINEL_F, SENTINEL_F, SENTINEL_C
    assert_bit_equal(d.cpu().numpy(), ed, f"{what}: direct")
    assert_bit_equal(i.cpu().numpy(), ei, f"{what}: indirect")
    assert np.array_equal(c.cpu().numpy(), ec), f"{what}: counts"
    if moments:
        assert_bit_equal(m.cpu().numpy(), em, f"{what}: moments")
    assert np.array_equal(r.cpu().numpy(), request), f"{what}: the request plane is read only"
    if counters is not None:
        for k in COUNTER_KEYS:
            assert ct[k] == counters[k], (what, k, ct, counters)
    return ct


def test_one_sample_everywhere_is_path_trace(gpu_ctx, cornell_small, cam, ref):
    from radish_pt_amd import api

    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_COUNT
    _use(gpu_ctx, cornell_small, cam)
    torch = _torch()
    ld, li = torch.zeros(P, 3, device="cuda"), torch.zeros(P, 3, device="cuda")
    gpu_ctx.counters_reset()
    gpu_ctx.path_trace(ld, li, 0, LOOPER, DEPTH, flags)
    want = gpu_ctx.counters()
    assert_bit_equal(ld.cpu().numpy(), ref["ad"][1], "path_trace vs oracle")
    ct = _run_and_check(gpu_ctx, ref, np.zeros(P, np.int32), np.ones(P, np.int32), flags, "all 1 over 0", counters=ref["stats"][0])
    assert ct == want


def test_equal_requests_are_path_trace_samples(gpu_ctx, cornell_small, cam, ref):
    from radish_pt_amd import api

    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT
    _use(gpu_ctx, cornell_small, cam)
    ld, li = _f(ref["ad"][3]), _f(ref["ai"][3])
    gpu_ctx.counters_reset()
    gpu_ctx.path_trace_samples(ld, li, 3, (LOOPER + 3) % 10000, 5, DEPTH, flags)
    want = gpu_ctx.counters()
    assert_bit_equal(ld.cpu().numpy(), ref["ad"][8], "path_trace_samples vs oracle")
    assert_bit_equal(li.cpu().numpy(), ref["ai"][8], "path_trace_samples vs oracle")
    stats = {k: sum(ref["stats"][n][k] for n in range(3, 8)) for k in COUNTER_KEYS}
    ct = _run_and_check(gpu_ctx, ref, np.full(P, 3, np.int32), np.full(P, 5, np.int32), flags, "all 5 over 3", counters=stats)
    assert ct == want


@pytest.fixture(scope="module")
def uneven_ref(cornell_small, cam):
    count, request = _uneven(20261)
    assert (request == 0).sum() > 8 * 16 and request.max() == 16 and len(np.unique(count)) == 8
    return count, request, ao.pair_counters(cornell_small, cam, LOOPER, count, request, DEPTH)


@pytest.mark.parametrize("flags_name", ["wavefront", "sort", "no_pairs", "small_lists", "walk_all"])
def test_uneven_requests_over_uneven_counts(gpu_ctx, cornell_small, cam, ref, uneven_ref, flags_name):
    from radish_pt_amd import api

    count, request, counters = uneven_ref
    _use(gpu_ctx, cornell_small, cam)
    _run_and_check(gpu_ctx, ref, count, request, _flags(api, flags_name) | api.RDH_PT_COUNT, f"uneven, {flags_name}", counters=counters)


def test_uneven_requests_without_counters_and_without_moments(gpu_ctx, cornell_small, cam, ref, uneven_ref):
    """The default launch (rays that cannot reach the image are not walked) and a null moments plane."""
    from radish_pt_amd import api

    count, request, _ = uneven_ref
    _use(gpu_ctx, cornell_small, cam)
    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_WF_SUBFRAMES  # (sub-frames: accepted and ignored)
    _run_and_check(gpu_ctx, ref, count, request, flags, "uneven, no counters")
    _run_and_check(gpu_ctx, ref, count, request, flags, "uneven, no moments", moments=False)


@pytest.mark.parametrize("total", [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1281])
def test_slot_totals_at_the_packet_edges(gpu_ctx, cornell_small, cam, ref, total):
    """One slot, the wave (64), the trace packet (128) and the shade and sort packets (256 .. 1 024, 1 281 = 1 024 + 256 + 1)."""
    from radish_pt_amd import api

    count, request = _plane_with_sum(total, total)
    _use(gpu_ctx, cornell_small, cam)
    _run_and_check(gpu_ctx, ref, count, request, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL, f"T = {total}")


def test_zero_plane_writes_nothing(gpu_ctx, cornell_small, cam, ref):
    from radish_pt_amd import api

    _use(gpu_ctx, cornell_small, cam)
    ct = _run_and_check(gpu_ctx, ref, np.zeros(P, np.int32), np.zeros(P, np.int32), api.RDH_PT_WAVEFRONT | api.RDH_PT_COUNT, "zero plane")
    assert all(v == 0 for v in ct.values()), ct


def test_one_pixel_frame(gpu_ctx, cornell_small):
    from radish_pt_amd import api, scenes

    cam1 = scenes.cornell_camera(1, 1)
    fr = ao.frames(cornell_small, cam1, LOOPER, 16, DEPTH)
    _use(gpu_ctx, cornell_small, cam1)
    stats = {k: sum(s[k] for s in fr["stats"]) for k in COUNTER_KEYS}
    _run_and_check(gpu_ctx, fr, np.zeros(1, np.int32), np.full(1, 16, np.int32), api.RDH_PT_WAVEFRONT | api.RDH_PT_COUNT, "1x1", counters=stats)


def test_scan_across_workgroup_totals(gpu_ctx, cornell_small):
    """256x257: 20 tiles of 64 blocks = 320 workgroups of 256 pixels, more than one tile of scanBlockTotals.  Requests at the first
    pixel, the last, one in the middle and one whole 8x8 block; the oracle renders just those pixels."""
    from oracle import pyoracle
    from radish_pt_amd import api, scenes

    w, h = 256, 257
    n = w * h
    cam2 = scenes.cornell_camera(w, h)
    rng = np.random.default_rng(5)
    request, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ys, xs = np.meshgrid(np.arange(136, 144), np.arange(72, 80), indexing="ij")
    picked = np.concatenate([[0, n - 1, 128 * w + 100], (ys * w + xs).reshape(-1)])
    request[picked] = rng.integers(1, 4, len(picked))
    count[picked] = rng.integers(0, 3, len(picked))
    orc = pyoracle.OracleScene(cornell_small)
    d0, i0 = np.full((n, 3), SENTINEL_F, np.float32), np.full((n, 3), SENTINEL_F, np.float32)
    m0, c0 = np.full((n, 2), SENTINEL_F, np.float32), np.full(n, SENTINEL_C, np.int32)
    d0[picked], i0[picked], m0[picked], c0[picked] = 0, 0, 0, count[picked]
    sd, si = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)

    def render(upto):
        """The oracle's means and the model's moments of the picked pixels after their first upto[p] samples."""
        d, i, m = d0.copy(), i0.copy(), m0.copy()
        for p in picked:
            for k in range(upto[p]):
                row, px = (LOOPER + k) % 10000, (int(p), int(p) + 1, 1)
                orc.path_trace(cam2, sd, si, 0, row, DEPTH, pix=px)  # iter 0 into any image: the finished sample itself
                L = am.luminance((sd[p] + si[p]).astype(np.float32))
                m[p, 0] = am.running_mean(m[p, 0], L, k)
                m[p, 1] = am.running_mean(m[p, 1], np.float32(L * L), k)
                orc.path_trace(cam2, d, i, k, row, DEPTH, pix=px)
        return d, i, m

    start = render(count)
    end = render(count + request)
    _use(gpu_ctx, cornell_small, cam2)
    d, i, m, c, r = _f(start[0]), _f(start[1]), _f(start[2]), _i(c0), _i(request)
    traced = gpu_ctx.path_trace_adaptive(d, i, c, r, LOOPER, DEPTH, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL, moments=m)
    assert traced == int(request.sum())
    ec = c0.copy()
    ec[picked] += request[picked]
    assert_bit_equal(d.cpu().numpy(), end[0], "256x257: direct")
    assert_bit_equal(i.cpu().numpy(), end[1], "256x257: indirect")
    assert_bit_equal(m.cpu().numpy(), end[2], "256x257: moments")
    assert np.array_equal(c.cpu().numpy(), ec)


def test_small_pass_after_a_large_one(gpu_ctx, cornell_small, cam, ref):
    """Two calls over one workspace: the second's total is far below the first's, so stale path state lies beyond it."""
    from radish_pt_amd import api

    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT
    _use(gpu_ctx, cornell_small, cam)
    _run_and_check(gpu_ctx, ref, np.full(P, 2, np.int32), np.full(P, 16, np.int32), flags, "large pass")
    count, request = _plane_with_sum(65, 99)
    counters = ao.pair_counters(cornell_small, cam, LOOPER, count, request, DEPTH)
    _run_and_check(gpu_ctx, ref, count, request, flags, "small pass after it", counters=counters)


def test_textured_scene_with_environment_map(gpu_ctx):
    from radish_pt_amd import api, scenes

    w, h, depth, looper = 40, 24, 3, 60
    sd = scenes.cornell_textured()
    camt = scenes.cornell_camera(w, h)
    fr = ao.frames(sd, camt, looper, NUM, depth)
    assert fr["ad"][1][0].max() > 0  # the corner pixel sees the environment map
    count, request = _uneven(77, w * h, w)
    _use(gpu_ctx, sd, camt)
    counters = ao.pair_counters(sd, camt, looper, count, request, depth)
    _run_and_check(gpu_ctx, fr, count, request, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT, "textured",
                   looper=looper, depth=depth, counters=counters)


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def _plan_and_check(ctx, count, moments, params, what):
    c, m = _i(count), _f(moments)
    r = _i(np.full(len(count), -9, np.int32))
    stats = ctx.adaptive_plan(c, m, r, params["min_samples"], params["max_samples"], params["step"], params["threshold"])
    want_r, want = am.plan(count, moments, W, H, **params)
    assert np.array_equal(r.cpu().numpy(), want_r), what
    assert stats == want, (what, stats, want)
    assert np.array_equal(c.cpu().numpy(), count)
    assert_bit_equal(m.cpu().numpy(), moments, f"{what}: the moments are read only")
    return want


def test_plan_equals_the_model(gpu_ctx, cornell_small, cam, ref):
    from radish_pt_amd import api

    _use(gpu_ctx, cornell_small, cam)
    torch = _torch()
    d, i, m = torch.zeros(P, 3, device="cuda"), torch.zeros(P, 3, device="cuda"), torch.zeros(P, 2, device="cuda")
    c, r = _i(np.zeros(P, np.int32)), _i(np.full(P, 8, np.int32))
    gpu_ctx.path_trace_adaptive(d, i, c, r, LOOPER, DEPTH, api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL, moments=m)
    counts, moments = c.cpu().numpy(), m.cpu().numpy()
    assert (counts == 8).all()
    assert_bit_equal(moments, ao.moments_after(ref, counts), "the GPU's moments after 8 uniform samples")
    want = _plan_and_check(gpu_ctx, counts, moments, {"min_samples": 4, "max_samples": 64, "step": 4, "threshold": PLAN_THRESHOLD},
                           "8 uniform samples")
    assert 0.2 <= want["activeBlocks"] / 35 <= 0.8, want
    hc, hm = am.hand_made_planes()
    _plan_and_check(gpu_ctx, hc, hm, am.HAND_PARAMS, "hand-made planes")
    # without `out` the call is asynchronous and fills the same plane
    c2, m2, r2 = _i(hc), _f(hm), _i(np.full(P, -9, np.int32))
    rc = api.adaptive_entries()[1](gpu_ctx.h, c2.data_ptr(), m2.data_ptr(), r2.data_ptr(), 4, 8, 4, 0.15, None)
    assert rc == 0
    gpu_ctx.synchronize()
    assert np.array_equal(r2.cpu().numpy(), am.plan(hc, hm, W, H, **am.HAND_PARAMS)[0])


def test_plan_refuses_bad_arguments(gpu_ctx, cornell_small, cam):
    from radish_pt_amd import api

    _use(gpu_ctx, cornell_small, cam)
    c, m, r = _i(np.zeros(P, np.int32)), _f(np.zeros((P, 2), np.float32)), _i(np.full(P, -9, np.int32))
    # (min_samples, max_samples, step, threshold)
    for name, (lo, hi, step, thr) in {"step 0": (1, 8, 0, 0.1), "step 17": (1, 8, 17, 0.1), "minSamples -1": (-1, 8, 4, 0.1),
                                      "max below min": (4, 3, 4, 0.1), "threshold -1": (1, 8, 4, -1.0),
                                      "threshold nan": (1, 8, 4, float("nan")), "threshold inf": (1, 8, 4, float("inf"))}.items():
        with pytest.raises(api.RadishError, match="error -1:"):
            gpu_ctx.adaptive_plan(c, m, r, lo, hi, step, thr)
    st = api.AdaptiveStatsC()
    for args in ((None, m.data_ptr(), r.data_ptr()), (c.data_ptr(), None, r.data_ptr()), (c.data_ptr(), m.data_ptr(), None)):
        assert api.adaptive_entries()[1](gpu_ctx.h, *args, 1, 8, 4, 0.1, C.byref(st)) == -1
    gpu_ctx.synchronize()
    assert (r.cpu().numpy() == -9).all()


# ---- converge --------------------------------------------------------------------------------------------------------------------
def test_converge_runs_three_passes_and_stops(gpu_ctx, cornell_small, cam, ref):
    """min 4, max 12, step 4: pass 1 samples everything (n < min), passes 2 and 3 the blocks the plan finds unsettled, and the fourth
    plan asks for nothing (what still wants is at the maximum).  Every pass is held to the oracle at the counts the model predicts
    from the oracle's own moments."""
    from radish_pt_amd import api

    params = {"min_samples": 4, "max_samples": 12, "step": 4, "threshold": PLAN_THRESHOLD}
    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL
    counts = np.zeros(P, np.int32)
    predicted = []  # (stats of the plan, counts after its pass)
    for _ in range(4):
        request, stats = am.plan(counts, ao.moments_after(ref, counts), W, H, **params)
        counts = counts + request
        predicted.append((stats, counts))
    assert [s["samplesRequested"] > 0 for s, _ in predicted] == [True, True, True, False]
    assert 0 < predicted[1][0]["activeBlocks"] < 35
    _use(gpu_ctx, cornell_small, cam)
    torch = _torch()
    for max_passes in (1, 2, 3, 10):
        d, i, m = torch.zeros(P, 3, device="cuda"), torch.zeros(P, 3, device="cuda"), torch.zeros(P, 2, device="cuda")
        c = _i(np.zeros(P, np.int32))
        passes = gpu_ctx.converge(d, i, c, m, LOOPER, DEPTH, flags, max_passes=max_passes, **params)
        ran = min(max_passes, 4)
        assert passes == [s for s, _ in predicted[:ran]], max_passes
        want = predicted[min(ran, 3) - 1][1]
        ed, ei = ao.means_at(ref, want)
        assert np.array_equal(c.cpu().numpy(), want), max_passes
        assert_bit_equal(d.cpu().numpy(), ed, f"converge, {max_passes} passes: direct")
        assert_bit_equal(i.cpu().numpy(), ei, f"converge, {max_passes} passes: indirect")
        assert_bit_equal(m.cpu().numpy(), ao.moments_after(ref, want), f"converge, {max_passes} passes: moments")


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_plane_untouched(gpu_ctx, cornell_small, cam, ref):
    from radish_pt_amd import api

    _use(gpu_ctx, cornell_small, cam)
    wf = api.RDH_PT_WAVEFRONT
    count, request = _plane_with_sum(300, 3)
    d0, i0 = ao.means_at(ref, count)
    m0 = ao.moments_after(ref, count)
    d, i, m = _f(d0), _f(i0), _f(m0)
    gpu_ctx.counters_reset()

    def refused(code, c_np, r_np, flags, looper=LOOPER, depth=DEPTH):
        c, r = _i(c_np), _i(r_np)
        with pytest.raises(api.RadishError, match=f"error {code}:"):
            gpu_ctx.path_trace_adaptive(d, i, c, r, looper, depth, flags | api.RDH_PT_COUNT, moments=m)
        assert np.array_equal(c.cpu().numpy(), c_np)

    first = int(np.flatnonzero(request > 0)[0])
    for name, (at, value) in {"a request of 17": ("r", 17), "a request of -1": ("r", -1), "a negative count": ("c", -1),
                              "count + request beyond int32": ("c", 2 ** 31 - 1)}.items():
        c_np, r_np = count.copy(), request.copy()
        (r_np if at == "r" else c_np)[first] = value
        refused(-1, c_np, r_np, wf)
    refused(-1, count, request, wf, looper=10000)
    refused(-1, count, request, wf, depth=29)
    refused(-3, count, request, 0)
    refused(-3, count, request, api.RDH_PT_PERSISTENT)
    refused(-3, count, request, wf | api.RDH_PT_PERSISTENT)
    refused(-3, count, request, api.RDH_PT_AUTO)
    refused(-3, count, request, wf | api.RDH_PT_AUTO)
    try:
        gpu_ctx.set_partition(1, 2, 64)
        refused(-3, count, request, wf)
    finally:
        gpu_ctx.set_partition(0, 1, 64)
    c, r = _i(count), _i(request)
    ptrs = [d.data_ptr(), i.data_ptr(), c.data_ptr(), r.data_ptr()]
    for k in range(4):  # null images, counts or requests (the moments may be null)
        args = list(ptrs)
        args[k] = None
        assert api.adaptive_entries()[0](gpu_ctx.h, *args, m.data_ptr(), LOOPER, DEPTH, wf, None) == -1
    gpu_ctx.synchronize()
    assert all(v == 0 for v in gpu_ctx.counters().values())  # nothing was traced
    assert_bit_equal(d.cpu().numpy(), d0, "direct after refused calls")
    assert_bit_equal(i.cpu().numpy(), i0, "indirect after refused calls")
    assert_bit_equal(m.cpu().numpy(), m0, "moments after refused calls")
    # and the context still renders
    _run_and_check(gpu_ctx, ref, count, request, wf, "after the refusals")


def test_total_beyond_the_slot_budget_is_refused(gpu_ctx, cornell_small):
    """1 024 x 1 024 pixels at 16 samples are 16.8 M slots, above what 4 GiB hold: refused after the scan, before any allocation
    for the pass (so the case costs two small launches), with T and the limit in the message."""
    from radish_pt_amd import api, scenes

    w = h = 1024
    _use(gpu_ctx, cornell_small, scenes.cornell_camera(w, h))
    torch = _torch()
    d, i = torch.full((w * h, 3), SENTINEL_F, device="cuda"), torch.full((w * h, 3), SENTINEL_F, device="cuda")
    c = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    r = torch.full((w * h,), 16, dtype=torch.int32, device="cuda")
    with pytest.raises(api.RadishError, match="error -1:") as e:
        gpu_ctx.path_trace_adaptive(d, i, c, r, LOOPER, DEPTH, api.RDH_PT_WAVEFRONT)
    assert str(w * h * 16) in str(e.value) and "2^30" in str(e.value), str(e.value)
    assert (d == SENTINEL_F).all().item() and (i == SENTINEL_F).all().item() and (c == 0).all().item()
