"""How a wavefront trace stage (k_wf_trace) hands its items out when workgroups have list duty (kernels_wave.h; DESIGN 5b, "A
workgroup with list duty takes no fixed share").  G = workgroups of the trace grid, L = min(list entries of the stage, G): the
workgroups with tickets below L trace a literal-class list entry together first and own no first packet, the waves of ticket
t >= L own packets 4 (t - L) .. 4 (t - L) + 3, and the shared head starts behind 4 (G - L) packets.

Which lane traces an item may change nothing: every case compares images bit for bit and the five RDH_PT_COUNT counters for
equality, against the CPU oracle on the whole frame.  Equal closestRays / anyRays is what shows that every item was traced
exactly once.

Two scenes.  `cornell_small` has next to no ray that looks literal-class (measured from the frames' own ray lists: none up to
256x192, 11 + 7 + 5 + 3 in the four stages of a 1920x1080 frame), so on it L = 0 and the cases only pin the unchanged path.  The
lists come from `flush_light`: the same scene with its lamp raised by 0.001 into the ceiling's plane, so that the shadow segment
of every path vertex on the ceiling has a y component of exactly zero or of an ulp — literal-looking, and both kinds occur: rays
the workgroup then traces whole, and rays for which the hint does not hold and which a lane takes.  The camera does not see the
ceiling, so the lists are those of stages 2 and 3.
  - 52x36, whole grid: some dozens of list entries and a few thousand items against ~6 000 first packets — 0 < L < G, most
    packets empty, duty workgroups that find the head dry;
  - a 64th of the grid (G <= 32: the persistent grid is capped at 2 048 workgroups), 160x120 and 256x192: the fixed packets
    cover at most 16 384 items of stage 1's ~20 000 / ~52 000, so the head hands out the rest, with the kind boundary and the end
    of the queue inside packets; against the oracle and against the whole grid;
  - the same with lists of four entries: 0 < L = 4 < G while the head is in use;
  - L == G: the flush-light frame at 256x192, whose stage 2 must hold at least 32 literal-looking rays (the test counts them
    itself, from the ray lists of depth 2 minus depth 1).  No frame of `cornell_small` of any practical size reaches that;
  - no lights (no shadow rays) and depth 1, at share 64.
"""
import numpy as np
import pytest

from helpers import assert_bit_equal, oracle_path_trace_mt

pytestmark = pytest.mark.gpu

COUNTER_KEYS = ("closestRays", "anyRays", "nodeVisits", "triTests", "closestHits")
DEPTH, LOOPER = 3, 7
WALKS = ("pairs", "threaded")
SIZES = ((160, 120), (256, 192))
GRID_CAP = 2048  # kPersistentGrid: workgroups of a persistent grid at share 1, at most


def _flags(api, walk, small_lists=False):
    f = api.RDH_PT_WAVEFRONT | api.RDH_PT_SORT_MATERIAL | api.RDH_PT_COUNT
    f |= {"pairs": api.RDH_PT_PAIRS, "threaded": api.RDH_PT_NO_PAIRS}[walk]
    return f | (api.RDH_PT_WF_SMALL_LISTS if small_lists else 0)


def _render(ctx, sd, cam, depth, flags, share=1):
    import torch

    w, h = (int(v) for v in cam["resolution"])
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    d, i = torch.zeros(w * h, 3, device="cuda"), torch.zeros(w * h, 3, device="cuda")
    try:
        ctx.set_occupancy_share(share)
        ctx.counters_reset()
        ctx.path_trace(d, i, 0, LOOPER, depth, flags)
        return d.cpu().numpy(), i.cpu().numpy(), ctx.counters()
    finally:
        ctx.set_occupancy_share(1)


def _check(got, ref, what):
    d, i, ct = got
    assert_bit_equal(d, ref["d"], f"{what}: direct vs oracle")
    assert_bit_equal(i, ref["i"], f"{what}: indirect vs oracle")
    for k in COUNTER_KEYS:
        assert ct[k] == ref["stats"][k], (what, k, ct[k], ref["stats"][k])


def _same(a, b, what):
    assert_bit_equal(a[0], b[0], f"{what}: direct")
    assert_bit_equal(a[1], b[1], f"{what}: indirect")
    assert a[2] == b[2], (what, a[2], b[2])


@pytest.fixture(scope="module")
def oracle_frames():
    """Oracle frames by (scene name, w, h, depth), computed once each and read-only."""
    from radish_pt_amd import scenes

    cache = {}

    def get(sd, w, h, depth):
        key = (sd.name, w, h, depth)
        if key not in cache:
            cam = scenes.cornell_camera(w, h)
            d, i = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
            _, st = oracle_path_trace_mt(sd, cam, d, i, 0, LOOPER, depth)
            d.setflags(write=False)
            i.setflags(write=False)
            cache[key] = {"cam": cam, "d": d, "i": i, "stats": {k: st[k] for k in COUNTER_KEYS}}
        return cache[key]

    return get


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


@pytest.fixture(scope="module")
def flush_light(cornell_small):
    """The Cornell scene with its lamp in the plane of the ceiling (y = 2) instead of 0.001 below it."""
    from radish_pt_amd import layouts as L, scenes

    lamps = [m for m in range(len(cornell_small.materials)) if cornell_small.materials[m]["type"] == L.LIGHT]
    v = np.array(cornell_small.vertices, dtype=np.float32).reshape(-1, 3, 3)
    lit = np.isin(np.asarray(cornell_small.material_ids), lamps)
    assert lit.sum() == 2 and np.all(v[lit, :, 1] == np.float32(1.999))
    v[lit, :, 1] = 2.0
    sd = scenes.SceneData("cornell_flush_light", v.reshape(-1, 3), cornell_small.normals, cornell_small.texcoords,
                          cornell_small.material_ids, cornell_small.materials.copy())
    assert sd.num_lights == 2
    return sd


@pytest.fixture(params=("cornell_small", "flush_light"))
def scene(request, cornell_small, flush_light):
    return {"cornell_small": cornell_small, "flush_light": flush_light}[request.param]


def _literal_looking(ctx, sd, cam, depth):
    """Rays and segments of the frame's ray lists that the hint takes for literal-class: a component below 1.1e-6 of the length."""
    ctx.set_partition(0, 1, 64)
    ctx.upload_scene(sd)
    ctx.set_camera(cam)
    rays, segs = ctx.dump_rays(LOOPER, depth)
    n = 0
    if rays.shape[0]:
        d = rays[:, 3:6].cpu().numpy().astype(np.float64)
        n += int((np.abs(d) < 1.1e-6 * np.linalg.norm(d, axis=1, keepdims=True)).any(axis=1).sum())
    if segs.shape[0]:
        s = segs.cpu().numpy().astype(np.float64)
        d = s[:, 3:6] - s[:, 0:3]
        n += int((np.abs(d) < 1.1e-6 * np.linalg.norm(d, axis=1, keepdims=True)).any(axis=1).sum())
    return n


@pytest.mark.parametrize("walk", WALKS)
def test_whole_grid_small_frame(gpu_ctx, scene, oracle_frames, walk):
    """52x36: far fewer items than first packets; with the flush light some dozens of list entries in stages 2 and 3."""
    from radish_pt_amd import api

    ref = oracle_frames(scene, 52, 36, DEPTH)
    assert ref["stats"]["anyRays"] > 0
    _check(_render(gpu_ctx, scene, ref["cam"], DEPTH, _flags(api, walk)), ref, f"{scene.name} 52x36, {walk}")


def test_flush_light_frames_have_lists(gpu_ctx, flush_light):
    """What the cases above and below rest on: stage 2 of the 52x36 flush-light frame has list entries, fewer than a grid."""
    from radish_pt_amd import scenes

    cam = scenes.cornell_camera(52, 36)
    n = _literal_looking(gpu_ctx, flush_light, cam, 2) - _literal_looking(gpu_ctx, flush_light, cam, 1)
    print(f"literal-looking rays of stage 2 at 52x36: {n}")
    assert 4 < n < 512, n


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("small_lists", (False, True), ids=("lists", "small_lists"))
@pytest.mark.parametrize("w,h", SIZES)
def test_sixty_fourth_of_the_grid(gpu_ctx, scene, oracle_frames, w, h, small_lists, walk):
    """Share 64 against the oracle and against share 1; the first packets must not cover stage 1 (so the head is in use)."""
    from radish_pt_amd import api

    ref = oracle_frames(scene, w, h, DEPTH)
    flags = _flags(api, walk, small_lists)
    fixed_max = (GRID_CAP // 64) * 4 * 128  # four waves' first packets per workgroup
    c0 = _render(gpu_ctx, scene, ref["cam"], 0, flags)[2]
    c1 = _render(gpu_ctx, scene, ref["cam"], 1, flags)[2]
    stage1 = (c1["closestRays"] - c0["closestRays"]) + (c1["anyRays"] - c0["anyRays"])
    assert stage1 > fixed_max, (stage1, fixed_max)
    whole = _render(gpu_ctx, scene, ref["cam"], DEPTH, flags)
    part = _render(gpu_ctx, scene, ref["cam"], DEPTH, flags, share=64)
    what = f"{scene.name} {w}x{h}, {walk}"
    _same(part, whole, f"{what}: share 64 vs share 1")
    _check(part, ref, f"{what}, share 64")
    _check(whole, ref, f"{what}, share 1")


@pytest.mark.parametrize("walk", WALKS)
def test_every_workgroup_has_list_duty(gpu_ctx, flush_light, oracle_frames, walk):
    """L == G: at share 64 the grid has at most 2 048 // 64 = 32 workgroups, so a stage with at least 32 list entries gives every
    workgroup list duty and nobody a first packet: everything goes through the head.  Stage 2 of the flush-light frame at 256x192
    must hold that many literal-looking rays: counted here with the hint's rule (a component below 1.1e-6 of the length) from the
    frame's own ray lists, depth 2 minus depth 1.  (`cornell_small` itself has none at this size and 7 in stage 1 at 1920x1080:
    its lamp is 0.001 below the ceiling, and the literal-looking rays of a frame grow with its edge, not its area.)"""
    from radish_pt_amd import api

    w, h = 256, 192
    ref = oracle_frames(flush_light, w, h, DEPTH)
    n = _literal_looking(gpu_ctx, flush_light, ref["cam"], 2) - _literal_looking(gpu_ctx, flush_light, ref["cam"], 1)
    print(f"literal-looking rays of stage 2 at {w}x{h}: {n}")
    assert n >= GRID_CAP // 64, (n, GRID_CAP // 64)
    _check(_render(gpu_ctx, flush_light, ref["cam"], DEPTH, _flags(api, walk), share=64), ref, f"L == G, {walk}")
    _check(_render(gpu_ctx, flush_light, ref["cam"], DEPTH, _flags(api, walk, small_lists=True), share=64), ref, f"L = 4 < G, {walk}")


@pytest.mark.parametrize("walk", WALKS)
def test_no_shadow_rays_at_share_64(gpu_ctx, unlit_scene, oracle_frames, walk):
    from radish_pt_amd import api

    ref = oracle_frames(unlit_scene, 160, 120, DEPTH)
    assert ref["stats"]["anyRays"] == 0 and ref["stats"]["closestRays"] > 160 * 120
    _check(_render(gpu_ctx, unlit_scene, ref["cam"], DEPTH, _flags(api, walk), share=64), ref, f"no lights, {walk}")


@pytest.mark.parametrize("walk", WALKS)
def test_depth_one_at_share_64(gpu_ctx, cornell_small, oracle_frames, walk):
    from radish_pt_amd import api

    ref = oracle_frames(cornell_small, 160, 120, 1)
    assert ref["stats"]["anyRays"] > 0
    total = ref["stats"]["closestRays"] - 160 * 120 + ref["stats"]["anyRays"]  # stage 1's items
    assert 16 < total % 128 < 112, total  # far from a multiple of the packet
    _check(_render(gpu_ctx, cornell_small, ref["cam"], 1, _flags(api, walk), share=64), ref, f"depth 1, {walk}")
