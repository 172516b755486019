"""Several samples per pixel in one call (rdh_path_trace_samples, Context.path_trace_samples).

Contract: the images and the work counters afterwards are bit for bit those of the host loop
    for s in range(samples): path_trace(d, i, iter + s, (looper + s) % 10000, depth, flags)
whatever the number of samples that share a wavefront pass (samples_per_pass), and so those of the CPU oracle.

The frame is 52x36: 7x5 = 35 8x8 blocks with partial blocks on both edges, and 35 B is no multiple of 4 for B = 1, 2, 3 and 5, so
the 4-wave workgroups of k_wf_raygen and k_wf_finish have ragged ends.  The batch starts at looper 9998, so the wrap of
State::looper to 0 lies inside it, on images that three ordinary path_trace calls have filled (iter 3: the running mean has weight).
"""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
W, H, DEPTH = 52, 36, 4
PRE_LOOPERS = (0, 1, 2)                   # iter 0..2: ordinary path_trace calls
ITER0, LOOPER0, SAMPLES = 3, 9998, 5      # the batch: iter 3..7, loopers 9998, 9999, 0, 1, 2


def _torch():
    import torch

    return torch


def _flags(api, name):
    return {"wavefront": api.RDH_PT_WAVEFRONT,
            "wavefront_sort": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL,
            "wavefront_small_lists": api.RDH_PT_WAVEFRONT | api.RDH_PT_WF_SMALL_LISTS,
            "wavefront_sort_pairs": api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_PAIRS,
            "wavefront_no_pairs": api.RDH_PT_WAVEFRONT | api.RDH_PT_NO_PAIRS}[name]


def _dev(a):
    return _torch().from_numpy(np.array(a, dtype=np.float32, copy=True)).cuda()  # the references stay read-only


def _loop(ctx, d, i, it0, looper0, samples, depth, flags):
    for s in range(samples):
        ctx.path_trace(d, i, it0 + s, (looper0 + s) % 10000, depth, flags)


def _use(ctx, sd, cam):
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)


@pytest.fixture(scope="module")
def oracle_ref(cornell_small):
    """The oracle's images after the three pre-fill frames and after all eight, and its work counters of the last five."""
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(W, H)
    d, i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    for it, looper in enumerate(PRE_LOOPERS):
        oracle_path_trace_mt(cornell_small, cam, d, i, it, looper, DEPTH)
    pre = (d.copy(), i.copy())
    stats = {k: 0 for k in COUNTER_KEYS}
    for s in range(SAMPLES):
        _, st = oracle_path_trace_mt(cornell_small, cam, d, i, ITER0 + s, (LOOPER0 + s) % 10000, DEPTH)
        for k in COUNTER_KEYS:
            stats[k] += st[k]
    assert d.max() > 0 and i.max() > 0
    for a in (pre[0], pre[1], d, i):
        a.setflags(write=False)
    return {"cam": cam, "pre": pre, "end": (d, i), "stats": stats}


@pytest.fixture(scope="module")
def loop_ref(gpu_ctx, cornell_small, oracle_ref):
    """The looped path_trace per flag set (pre-fill included), computed once each."""
    from radish_pt_amd import api

    cache = {}

    def get(name):
        if name not in cache:
            flags = _flags(api, name) | api.RDH_PT_COUNT
            _use(gpu_ctx, cornell_small, oracle_ref["cam"])
            d, i = _torch().zeros(W * H, 3, device="cuda"), _torch().zeros(W * H, 3, device="cuda")
            for it, looper in enumerate(PRE_LOOPERS):
                gpu_ctx.path_trace(d, i, it, looper, DEPTH, flags)
            pre = (d.cpu().numpy(), i.cpu().numpy())
            gpu_ctx.counters_reset()
            _loop(gpu_ctx, d, i, ITER0, LOOPER0, SAMPLES, DEPTH, flags)
            cache[name] = {"pre": pre, "end": (d.cpu().numpy(), i.cpu().numpy()), "counters": gpu_ctx.counters()}
        return cache[name]

    return get


@pytest.mark.parametrize("samples_per_pass", [0, 1, 2, 5, 9])  # 2: passes of 2, 2, 1; 9: clamped to 5
@pytest.mark.parametrize("flags_name", ["wavefront", "wavefront_sort", "wavefront_small_lists", "wavefront_sort_pairs", "wavefront_no_pairs"])
def test_samples_equal_the_loop_and_the_oracle(gpu_ctx, cornell_small, oracle_ref, loop_ref, flags_name, samples_per_pass):
    from radish_pt_amd import api

    flags = _flags(api, flags_name) | api.RDH_PT_COUNT
    loop = loop_ref(flags_name)
    assert_bit_equal(loop["pre"][0], oracle_ref["pre"][0], "pre-fill direct vs oracle")
    assert_bit_equal(loop["pre"][1], oracle_ref["pre"][1], "pre-fill indirect vs oracle")
    _use(gpu_ctx, cornell_small, oracle_ref["cam"])
    d, i = _dev(loop["pre"][0]), _dev(loop["pre"][1])
    gpu_ctx.counters_reset()
    gpu_ctx.path_trace_samples(d, i, ITER0, LOOPER0, SAMPLES, DEPTH, flags, samples_per_pass=samples_per_pass)
    got_d, got_i, ct = d.cpu().numpy(), i.cpu().numpy(), gpu_ctx.counters()
    what = f"{flags_name}, samples_per_pass={samples_per_pass}"
    assert_bit_equal(got_d, loop["end"][0], f"{what}: direct vs loop")
    assert_bit_equal(got_i, loop["end"][1], f"{what}: indirect vs loop")
    assert_bit_equal(got_d, oracle_ref["end"][0], f"{what}: direct vs oracle")
    assert_bit_equal(got_i, oracle_ref["end"][1], f"{what}: indirect vs oracle")
    assert ct == loop["counters"], what
    for k in COUNTER_KEYS:
        assert ct[k] == oracle_ref["stats"][k], (what, k)


def test_textured_scene_with_environment_map(gpu_ctx):
    """The miss / env-map MIS terms land in the same accumulators: three samples in one pass."""
    from radish_pt_amd import api, scenes

    w, h, depth, samples, looper0 = 40, 24, 3, 3, 60
    sd = scenes.cornell_textured()
    cam = scenes.cornell_camera(w, h)
    ref_d, ref_i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    stats = {k: 0 for k in COUNTER_KEYS}
    for s in range(samples):
        _, st = oracle_path_trace_mt(sd, cam, ref_d, ref_i, s, looper0 + s, depth)
        for k in COUNTER_KEYS:
            stats[k] += st[k]
    assert ref_d[0].max() > 0  # the corner pixel sees the environment map
    _use(gpu_ctx, sd, cam)
    torch = _torch()
    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT
    ld, li = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    _loop(gpu_ctx, ld, li, 0, looper0, samples, depth, flags)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    gpu_ctx.counters_reset()
    gpu_ctx.path_trace_samples(d, i, 0, looper0, samples, depth, flags, samples_per_pass=3)
    ct = gpu_ctx.counters()
    assert_bit_equal(d.cpu().numpy(), ld.cpu().numpy(), "textured: direct vs loop")
    assert_bit_equal(i.cpu().numpy(), li.cpu().numpy(), "textured: indirect vs loop")
    assert_bit_equal(d.cpu().numpy(), ref_d, "textured: direct vs oracle")
    assert_bit_equal(i.cpu().numpy(), ref_i, "textured: indirect vs oracle")
    for k in COUNTER_KEYS:
        assert ct[k] == stats[k], k


def test_tile_partition(gpu_ctx, cornell_small):
    """Rank 1 of 3 at 200x136 (12 tiles of 64, four of them this rank's): packed tiles, as path_trace writes them."""
    from radish_pt_amd import api, scenes

    w, h, depth, samples = 200, 136, 4, 3
    torch = _torch()
    flags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT
    _use(gpu_ctx, cornell_small, scenes.cornell_camera(w, h))
    try:
        gpu_ctx.set_partition(1, 3, 64)
        n = gpu_ctx.tiles_per_rank() * 64 * 64
        ld, li = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
        gpu_ctx.counters_reset()
        _loop(gpu_ctx, ld, li, 0, 9999, samples, depth, flags)
        want = gpu_ctx.counters()
        assert ld.max().item() > 0
        for spp in (3, 2):
            d, i = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
            gpu_ctx.counters_reset()
            gpu_ctx.path_trace_samples(d, i, 0, 9999, samples, depth, flags, samples_per_pass=spp)
            assert_bit_equal(d.cpu().numpy(), ld.cpu().numpy(), f"partition, samples_per_pass={spp}: direct")
            assert_bit_equal(i.cpu().numpy(), li.cpu().numpy(), f"partition, samples_per_pass={spp}: indirect")
            assert gpu_ctx.counters() == want, spp
    finally:
        gpu_ctx.set_partition(0, 1, 64)


@pytest.mark.parametrize("structure", ["persistent", "megakernel"])
def test_other_structures_run_the_samples_one_launch_each(gpu_ctx, cornell_small, oracle_ref, structure):
    from radish_pt_amd import api

    flags = {"persistent": api.RDH_PT_PERSISTENT, "megakernel": api.RDH_PT_MEGAKERNEL}[structure] | api.RDH_PT_COUNT
    torch = _torch()
    _use(gpu_ctx, cornell_small, oracle_ref["cam"])
    ld, li = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    gpu_ctx.counters_reset()
    _loop(gpu_ctx, ld, li, 0, 9998, 4, DEPTH, flags)
    want = gpu_ctx.counters()
    d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
    gpu_ctx.counters_reset()
    gpu_ctx.path_trace_samples(d, i, 0, 9998, 4, DEPTH, flags, samples_per_pass=3)  # ignored by these structures
    assert_bit_equal(d.cpu().numpy(), ld.cpu().numpy(), f"{structure}: direct")
    assert_bit_equal(i.cpu().numpy(), li.cpu().numpy(), f"{structure}: indirect")
    assert gpu_ctx.counters() == want


@pytest.mark.parametrize("structure", ["wavefront", "persistent", "megakernel", "auto"])
def test_one_sample_is_path_trace(gpu_ctx, cornell_small, oracle_ref, structure):
    from radish_pt_amd import api

    flags = {"wavefront": api.RDH_PT_WAVEFRONT, "persistent": api.RDH_PT_PERSISTENT, "megakernel": api.RDH_PT_MEGAKERNEL,
             "auto": api.RDH_PT_AUTO}[structure]
    _use(gpu_ctx, cornell_small, oracle_ref["cam"])
    ld, li = _dev(oracle_ref["pre"][0]), _dev(oracle_ref["pre"][1])
    gpu_ctx.path_trace(ld, li, 3, 9999, DEPTH, flags)
    d, i = _dev(oracle_ref["pre"][0]), _dev(oracle_ref["pre"][1])
    gpu_ctx.path_trace_samples(d, i, 3, 9999, 1, DEPTH, flags)
    assert_bit_equal(d.cpu().numpy(), ld.cpu().numpy(), f"{structure}: direct")
    assert_bit_equal(i.cpu().numpy(), li.cpu().numpy(), f"{structure}: indirect")


def test_module_level_mirror_advances_the_looper(cornell_small, oracle_ref):
    """pathTraceSamples beside pathTrace: reads Settings.traceDepth, advances State.looper `samples` times (with the wrap)."""
    from radish_pt_amd import api

    torch = _torch()
    saved = (api.State.scene, api.State.looper, api.Settings.traceDepth, api.Settings.ptFlags)
    scene = api.Scene(cornell_small, oracle_ref["cam"])
    try:
        api.State.scene = scene
        api.Settings.traceDepth = DEPTH
        api.Settings.ptFlags = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL
        api.State.looper = PRE_LOOPERS[0]
        d, i = torch.zeros(W * H, 3, device="cuda"), torch.zeros(W * H, 3, device="cuda")
        api.pathTraceSamples(d, i, 0, len(PRE_LOOPERS))
        assert api.State.looper == PRE_LOOPERS[-1] + 1
        assert_bit_equal(d.cpu().numpy(), oracle_ref["pre"][0], "pathTraceSamples, pre-fill: direct")
        api.State.looper = LOOPER0
        api.pathTraceSamples(d, i, ITER0, SAMPLES)
        assert api.State.looper == (LOOPER0 + SAMPLES) % 10000
        assert_bit_equal(d.cpu().numpy(), oracle_ref["end"][0], "pathTraceSamples: direct")
        assert_bit_equal(i.cpu().numpy(), oracle_ref["end"][1], "pathTraceSamples: indirect")
    finally:
        scene.clear()
        api.State.scene, api.State.looper, api.Settings.traceDepth, api.Settings.ptFlags = saved


def test_errors_leave_the_images_untouched(gpu_ctx, cornell_small, oracle_ref):
    from radish_pt_amd import api

    _use(gpu_ctx, cornell_small, oracle_ref["cam"])
    d, i = _dev(oracle_ref["pre"][0]), _dev(oracle_ref["pre"][1])
    wf = api.RDH_PT_WAVEFRONT
    over = (1 << 30) // (35 * 64) + 1  # one more sample than 2^30 slots hold on this frame: refused before any allocation
    # (iter, looper, samples, depth, samples_per_pass)
    cases = {"numSamples 0": (3, 0, 0, DEPTH, 0), "samples_per_pass -1": (3, 0, 2, DEPTH, -1), "looper 10000": (3, 10000, 2, DEPTH, 0),
             "depth 29": (3, 0, 2, 29, 0), "samples_per_pass above the slot cap": (3, 0, over, DEPTH, over)}
    for name, (it, looper, samples, depth, spp) in cases.items():
        for flags in (wf, wf | api.RDH_PT_SORT_MATERIAL, api.RDH_PT_PERSISTENT, api.RDH_PT_MEGAKERNEL):
            if "slot cap" in name and not flags & wf:
                continue  # those structures take one sample per launch and ignore samples_per_pass
            with pytest.raises(api.RadishError, match="error -1:") as e:  # RDH_ERR_ARGS
                gpu_ctx.path_trace_samples(d, i, it, looper, samples, depth, flags, samples_per_pass=spp)
            if "slot cap" in name:
                assert "2^30" in str(e.value), str(e.value)
    gpu_ctx.synchronize()
    assert_bit_equal(d.cpu().numpy(), oracle_ref["pre"][0], "direct after refused calls")
    assert_bit_equal(i.cpu().numpy(), oracle_ref["pre"][1], "indirect after refused calls")
    # and the context still renders
    gpu_ctx.path_trace_samples(d, i, ITER0, LOOPER0, SAMPLES, DEPTH, wf)
    assert_bit_equal(d.cpu().numpy(), oracle_ref["end"][0], "direct after the errors")
